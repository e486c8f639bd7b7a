// drt_decode.hip -- Gray-code pattern photographs -> screen codes, contrast, silhouette mask and ray targets on the device (drt_decode.h
// holds the law).  One fused streaming pass: every input byte is read once and every output written once, no
// workspace, no LDS, no atomics -- the same inputs give the same bits.  The kernel is bound by HBM bytes (F or 2 F in, about 30 out per
// pixel), so a lane owns a run of kDecodeRun adjacent pixels of one view and reads each frame's run as one machine word.
#include "drt_device.h"
#include "drt_decode.h"

#ifndef DRT_DECODE_RUN
#define DRT_DECODE_RUN 8                         // pixels per lane: 4 (dword loads) or 8 (dwordx2); measurement variants override it
#endif
#ifndef DRT_DECODE_INFLIGHT
#define DRT_DECODE_INFLIGHT 4                    // bits whose two frames are loaded before the first compare
#endif

namespace {

constexpr int kDecodeBlock = 256;
constexpr int kDecodeRun = DRT_DECODE_RUN;
constexpr int kDecodeBatch = DRT_DECODE_INFLIGHT;
static_assert(kDecodeRun == 4 || kDecodeRun == 8, "a run is one dword or two");
static_assert(kDecodeBatch >= 1 && kDecodeBatch <= 8, "frames in flight");

template <int N> struct RunWord;
template <> struct RunWord<4> { using type = uint32_t; };
template <> struct RunWord<8> { using type = uint64_t; };
using Word = RunWord<kDecodeRun>::type;

// One stack of photographs: this view's frame 0, and how many bytes of the whole allocation lie before it and from it to the end: no
// load may leave [view - before, view + after).
struct DecodeStack {
    const uint8_t* view;
    int64_t before;
    int64_t after;
};

// The run [p0, p0 + kDecodeRun) of the plane that starts at `plane`, as a little-endian word.  `plane` is wave-uniform and p0 a multiple
// of the word size, so the misalignment s of the run is that of the plane: a scalar.  ALIGNED (chosen per launch from the real
// addresses): every plane starts on a word boundary, one load.  Otherwise two aligned loads around the run and a funnel shift; the
// caller has checked that both stay inside the stack.  Neither form has a branch, so a batch of them issues back to back.
template <bool ALIGNED>
__device__ __forceinline__ Word load_run(const uint8_t* __restrict__ plane, int64_t p0) {
    if (ALIGNED) return *reinterpret_cast<const Word*>(plane + p0);
    const unsigned s = (unsigned)(reinterpret_cast<uintptr_t>(plane) & (kDecodeRun - 1));
    const uint8_t* a = plane + p0 - s;
    const Word w0 = *reinterpret_cast<const Word*>(a);
    const Word w1 = *reinterpret_cast<const Word*>(a + (s ? kDecodeRun : 0));
    return s ? (Word)((w0 >> (8 * s)) | (w1 << (8 * (kDecodeRun - s)))) : w0;
}

// Heads and tails: the first n bytes of the run, one at a time (the others read as 0 and are never stored).
__device__ __forceinline__ Word load_run_bytes(const uint8_t* __restrict__ plane, int64_t p0, int n) {
    Word w = 0;
#pragma unroll
    for (int j = 0; j < kDecodeRun; ++j)
        if (j < n) w |= (Word)plane[p0 + j] << (8 * j);
    return w;
}

// Codes of the run's pixels from one stack: kDecodeBatch bits (2 kDecodeBatch frames) are loaded before the first compare.  A frame
// index beyond the stack is clamped to the last frame (a repeated load, not used), so the load sequence has no branch.
template <bool ALIGNED>
__device__ __forceinline__ void decode_run(const DecodeLaw& L, const DecodeStack& S, int64_t plane, int64_t p0, int n, int (&x)[kDecodeRun],
                                           int (&y)[kDecodeRun], int (&contrast)[kDecodeRun], bool (&ok)[kDecodeRun]) {
    const int n_bits = L.nbx + L.nby, last = 2 * n_bits - 1;
    // wide loads need the whole run inside the plane; the two-load form also reads up to one word before and after the run
    const bool wide = n == kDecodeRun && (ALIGNED || (S.before + p0 >= kDecodeRun && (int64_t)last * plane + p0 + 2 * kDecodeRun <= S.after));
    unsigned gray[kDecodeRun];
#pragma unroll
    for (int j = 0; j < kDecodeRun; ++j) { gray[j] = 0; contrast[j] = 255; }
    for (int t0 = 0; t0 < n_bits; t0 += kDecodeBatch) {
        Word w[2 * kDecodeBatch];
        if (wide) {
#pragma unroll
            for (int i = 0; i < 2 * kDecodeBatch; ++i) {
                const int f = 2 * t0 + i < last ? 2 * t0 + i : last;
                w[i] = load_run<ALIGNED>(S.view + (int64_t)f * plane, p0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2 * kDecodeBatch; ++i) {
                const int f = 2 * t0 + i < last ? 2 * t0 + i : last;
                w[i] = load_run_bytes(S.view + (int64_t)f * plane, p0, n);
            }
        }
#pragma unroll
        for (int i = 0; i < kDecodeBatch; ++i) {
            if (t0 + i >= n_bits) break;
#pragma unroll
            for (int j = 0; j < kDecodeRun; ++j)
                decode_bit(gray[j], contrast[j], (int)((w[2 * i] >> (8 * j)) & 0xffu), (int)((w[2 * i + 1] >> (8 * j)) & 0xffu));
        }
    }
#pragma unroll
    for (int j = 0; j < kDecodeRun; ++j) ok[j] = decode_code(L, gray[j], contrast[j], x[j], y[j]);
}

// A run of bytes: one word when the view's plane of this output starts on a word boundary and the run is whole.
__device__ __forceinline__ void store_bytes(uint8_t* __restrict__ plane, int64_t p0, int n, const uint8_t (&v)[kDecodeRun]) {
    if (n == kDecodeRun && (reinterpret_cast<uintptr_t>(plane) & (kDecodeRun - 1)) == 0) {
        Word w = 0;
#pragma unroll
        for (int j = 0; j < kDecodeRun; ++j) w |= (Word)v[j] << (8 * j);
        *reinterpret_cast<Word*>(plane + p0) = w;
        return;
    }
#pragma unroll
    for (int j = 0; j < kDecodeRun; ++j)
        if (j < n) plane[p0 + j] = v[j];
}

}  // namespace

// grid.y = view, grid.x = blocks of kDecodeBlock runs of the view's H W pixels.  The view's screen is read through a uniform address:
// nine doubles in scalar registers.
template <bool ALIGNED>
__global__ void __launch_bounds__(kDecodeBlock) k_decode_patterns(DecodeLaw L, const uint8_t* __restrict__ frames, const uint8_t* __restrict__ background,
                                                                  int64_t background_view_stride, int n_views, int64_t plane,
                                                                  const double* __restrict__ screens, int zero_outside_mask, int16_t* __restrict__ codes,
                                                                  uint8_t* __restrict__ contrast_out, uint8_t* __restrict__ mask_out,
                                                                  uint8_t* __restrict__ covered_out, double* __restrict__ positions) {
    const int view = blockIdx.y;
    const int64_t p0 = ((int64_t)blockIdx.x * kDecodeBlock + threadIdx.x) * kDecodeRun;
    if (p0 >= plane) return;
    const int n = plane - p0 < kDecodeRun ? (int)(plane - p0) : kDecodeRun;
    const int n_frames = 2 * (L.nbx + L.nby);
    const int64_t view_bytes = (int64_t)n_frames * plane;

    int x[kDecodeRun], y[kDecodeRun], contrast[kDecodeRun];
    bool ok[kDecodeRun];
    const DecodeStack obj{frames + view * view_bytes, view * view_bytes, (n_views - view) * view_bytes};
    decode_run<ALIGNED>(L, obj, plane, p0, n, x, y, contrast, ok);

    uint8_t mask[kDecodeRun];
#pragma unroll
    for (int j = 0; j < kDecodeRun; ++j) mask[j] = 255;                        // without a background nothing is outside the mask
    if (background) {
        int xb[kDecodeRun], yb[kDecodeRun], cb[kDecodeRun];
        bool okb[kDecodeRun];
        const int64_t bg_before = view * background_view_stride;                 // 0 for a shared background
        const DecodeStack bg{background + bg_before, bg_before, (background_view_stride ? (n_views - 1) * background_view_stride : 0) + view_bytes - bg_before};
        decode_run<ALIGNED>(L, bg, plane, p0, n, xb, yb, cb, okb);
        uint8_t covered[kDecodeRun];
#pragma unroll
        for (int j = 0; j < kDecodeRun; ++j) {
            mask[j] = decode_mask(L, ok[j], x[j], y[j], okb[j], xb[j], yb[j]);
            covered[j] = okb[j] ? 1 : 0;
        }
        if (mask_out) store_bytes(mask_out + view * plane, p0, n, mask);
        if (covered_out) store_bytes(covered_out + view * plane, p0, n, covered);
    }

    const int64_t pix = view * plane + p0;                                       // first pixel of the run in the [n, H W] outputs
    {
        uint8_t c8[kDecodeRun];
#pragma unroll
        for (int j = 0; j < kDecodeRun; ++j) c8[j] = (uint8_t)contrast[j];
        store_bytes(contrast_out + view * plane, p0, n, c8);
    }
    {
        int16_t* dst = codes + 2 * pix;
        if (n == kDecodeRun && (reinterpret_cast<uintptr_t>(codes + 2 * view * plane) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < kDecodeRun / 4; ++q) {
                uint4 v;
                v.x = ((unsigned)x[4 * q] & 0xffffu) | ((unsigned)y[4 * q] << 16);
                v.y = ((unsigned)x[4 * q + 1] & 0xffffu) | ((unsigned)y[4 * q + 1] << 16);
                v.z = ((unsigned)x[4 * q + 2] & 0xffffu) | ((unsigned)y[4 * q + 2] << 16);
                v.w = ((unsigned)x[4 * q + 3] & 0xffffu) | ((unsigned)y[4 * q + 3] << 16);
                reinterpret_cast<uint4*>(dst)[q] = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kDecodeRun; ++j)
                if (j < n) { dst[2 * j] = (int16_t)x[j]; dst[2 * j + 1] = (int16_t)y[j]; }
        }
    }
    if (positions) {
        double sc[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) sc[c] = screens[9 * view + c];
        double p[3 * kDecodeRun];
#pragma unroll
        for (int j = 0; j < kDecodeRun; ++j) {
            const bool keep = ok[j] && !(zero_outside_mask && mask[j] == 0);
            double q[3];
            decode_position(sc, x[j], y[j], q);
            p[3 * j] = keep ? q[0] : 0.0; p[3 * j + 1] = keep ? q[1] : 0.0; p[3 * j + 2] = keep ? q[2] : 0.0;
        }
        double* dst = positions + 3 * pix;
        if (n == kDecodeRun && (reinterpret_cast<uintptr_t>(positions + 3 * view * plane) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < 3 * kDecodeRun / 2; ++q) reinterpret_cast<double2*>(dst)[q] = double2{p[2 * q], p[2 * q + 1]};
        } else {
#pragma unroll
            for (int j = 0; j < 3 * kDecodeRun; ++j)
                if (j < 3 * n) dst[j] = p[j];
        }
    }
}

extern "C" {

int drt_decode_patterns(const uint8_t* d_frames, const uint8_t* d_background, int64_t background_view_stride, int n_views, int height, int width,
                        int tex_h, int tex_w, int min_contrast, int mask_shift, const double* d_screens, int zero_outside_mask, int16_t* d_codes,
                        uint8_t* d_contrast, uint8_t* d_mask, uint8_t* d_covered, double* d_positions, void* stream) {
    if (!d_frames) return fail(DRT_E_INVALID, "d_frames is null");
    if (n_views < 1 || n_views > 65535) return fail(DRT_E_INVALID, "n_views = %d: must be in [1, 65535]", n_views);
    if (height < 1 || width < 1) return fail(DRT_E_INVALID, "height x width = %d x %d: photographs must be at least 1 x 1", height, width);
    if (tex_h < 2 || tex_h > kDecodeMaxTex) return fail(DRT_E_INVALID, "tex_h = %d: must be in [2, %d]", tex_h, kDecodeMaxTex);
    if (tex_w < 2 || tex_w > kDecodeMaxTex) return fail(DRT_E_INVALID, "tex_w = %d: must be in [2, %d]", tex_w, kDecodeMaxTex);
    if (min_contrast < 1 || min_contrast > 255) return fail(DRT_E_INVALID, "min_contrast = %d: must be in [1, 255]", min_contrast);
    if (mask_shift < 1 || mask_shift > kDecodeMaxTex) return fail(DRT_E_INVALID, "mask_shift = %d: must be in [1, %d]", mask_shift, kDecodeMaxTex);
    if (zero_outside_mask != 0 && zero_outside_mask != 1) return fail(DRT_E_INVALID, "zero_outside_mask = %d: 0 or 1", zero_outside_mask);
    const int64_t plane = (int64_t)height * width;
    const int64_t view_bytes = (int64_t)decode_frames(tex_h, tex_w) * plane;
    if (background_view_stride != 0 && background_view_stride < view_bytes)
        return fail(DRT_E_INVALID, "background_view_stride = %lld: 0 (one background for all views) or at least the %lld bytes of a view's frames",
                    (long long)background_view_stride, (long long)view_bytes);
    if (!d_background && background_view_stride != 0) return fail(DRT_E_INVALID, "background_view_stride is set but d_background is null");
    if (!d_background && (d_mask || d_covered)) return fail(DRT_E_INVALID, "d_mask / d_covered need d_background");
    if (!d_background && zero_outside_mask) return fail(DRT_E_INVALID, "zero_outside_mask needs d_background");
    if (d_positions && !d_screens) return fail(DRT_E_INVALID, "d_positions needs d_screens");
    if (zero_outside_mask && !d_positions) return fail(DRT_E_INVALID, "zero_outside_mask needs d_positions");
    if (!d_codes) return fail(DRT_E_INVALID, "d_codes is null");
    if (!d_contrast) return fail(DRT_E_INVALID, "d_contrast is null");
    if ((reinterpret_cast<uintptr_t>(d_codes) & 1) != 0) return fail(DRT_E_INVALID, "d_codes must be aligned to its int16 elements");
    if ((reinterpret_cast<uintptr_t>(d_positions) & 7) != 0) return fail(DRT_E_INVALID, "d_positions must be aligned to its float64 elements");
    if ((reinterpret_cast<uintptr_t>(d_screens) & 7) != 0) return fail(DRT_E_INVALID, "d_screens must be aligned to its float64 elements");
    const DecodeLaw L = decode_law(tex_h, tex_w, min_contrast, mask_shift);
    const int64_t run_block = (int64_t)kDecodeBlock * kDecodeRun;
    const dim3 grid((unsigned)((plane + run_block - 1) / run_block), (unsigned)n_views);
    // one load per run where every plane of both stacks starts on a word boundary; otherwise the two-load form for all of them
    const bool aligned = (reinterpret_cast<uintptr_t>(d_frames) % kDecodeRun) == 0 && plane % kDecodeRun == 0 &&
                         (!d_background || ((reinterpret_cast<uintptr_t>(d_background) % kDecodeRun) == 0 && background_view_stride % kDecodeRun == 0));
    if (aligned)
        k_decode_patterns<true><<<grid, kDecodeBlock, 0, (hipStream_t)stream>>>(L, d_frames, d_background, background_view_stride, n_views, plane, d_screens,
                                                                                zero_outside_mask, d_codes, d_contrast, d_mask, d_covered, d_positions);
    else
        k_decode_patterns<false><<<grid, kDecodeBlock, 0, (hipStream_t)stream>>>(L, d_frames, d_background, background_view_stride, n_views, plane, d_screens,
                                                                                 zero_outside_mask, d_codes, d_contrast, d_mask, d_covered, d_positions);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

}  // extern "C"
