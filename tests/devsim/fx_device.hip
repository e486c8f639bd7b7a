// tests/devsim/fx_device.hip -- test-only: the deterministic-mode accumulators of drt_fixed.h / drt_device.h / drt_pathsink.h launched
// ALONE on the device, so that tests/test_gpu_fixed_device.py can hold their cells against Python integers.  What tests/hostsim is to the
// host compilation of the shared headers, this is to the gfx950 one.  The production structs are used unchanged -- there is no copy of
// their logic here, only the loops around them -- and nothing of this file is part of libdrt_hip.so or of its C ABI.
// The callers validate every index against the size of the target before a launch; the kernels do not.
#include "drt_pathsink.h"

using namespace drt;

// GradAdd3<true>: two global integer atomics per component, no table
__global__ void __launch_bounds__(256) k_dv_direct(double* cells, const int32_t* __restrict__ idx, const double* __restrict__ x, int64_t n) {
    const GradAdd3<true> add{cells};
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        add(idx[i], d3{x[3 * i], x[3 * i + 1], x[3 * i + 2]});
}

// the batch loop of k_loss_bwd_fused (drt_pipeline.hip) around PathSink<DET>, with the batch size as an argument
template <bool DET>
__global__ void __launch_bounds__(256) k_dv_sink(double* target, const int32_t* __restrict__ idx, const double* __restrict__ x, int64_t n, int64_t batch) {
    __shared__ int32_t hkeys[kHashSize];
    __shared__ double hsums[3 * kHashSize];
    const PathSink<DET> add{hkeys, hsums, target};
    for (int64_t base = blockIdx.x * batch; base < n; base += (int64_t)gridDim.x * batch) {
        add.clear();
        const int64_t end = base + batch < n ? base + batch : n;
        for (int64_t k = base + threadIdx.x; k < end; k += blockDim.x) add(idx[k], d3{x[3 * k], x[3 * k + 1], x[3 * k + 2]});
        add.flush();
    }
}

// LossAcc<true>: per thread, per wave, one atomic pair per wave; every thread reaches the flush
__global__ void __launch_bounds__(256) k_dv_loss(double* cell, const double* __restrict__ x, int64_t n) {
    LossAcc<true> acc;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc.add(x[i]);
    acc.flush(cell);
}

extern "C" {

int dv_direct(void* d_cells, const int32_t* d_idx, const double* d_x, int64_t n, int grid, void* stream) {
    if (n <= 0 || grid <= 0) return (int)hipSuccess;
    k_dv_direct<<<grid, 256, 0, (hipStream_t)stream>>>(static_cast<double*>(d_cells), d_idx, d_x, n);
    return (int)hipGetLastError();
}
int dv_sink_det(void* d_cells, const int32_t* d_idx, const double* d_x, int64_t n, int64_t batch, int grid, void* stream) {
    if (n <= 0 || grid <= 0 || batch <= 0) return (int)hipSuccess;
    k_dv_sink<true><<<grid, 256, 0, (hipStream_t)stream>>>(static_cast<double*>(d_cells), d_idx, d_x, n, batch);
    return (int)hipGetLastError();
}
int dv_sink_f64(double* d_g, const int32_t* d_idx, const double* d_x, int64_t n, int64_t batch, int grid, void* stream) {
    if (n <= 0 || grid <= 0 || batch <= 0) return (int)hipSuccess;
    k_dv_sink<false><<<grid, 256, 0, (hipStream_t)stream>>>(d_g, d_idx, d_x, n, batch);
    return (int)hipGetLastError();
}
int dv_loss(void* d_cell, const double* d_x, int64_t n, int grid, void* stream) {
    if (n <= 0 || grid <= 0) return (int)hipSuccess;
    k_dv_loss<<<grid, 256, 0, (hipStream_t)stream>>>(static_cast<double*>(d_cell), d_x, n);
    return (int)hipGetLastError();
}

}  // extern "C"
