// drt_image_views.h -- the image term of several views in one call (drt_render_image_loss_views): where a sample's
// camera and screen come from, and how a row of the band maps to (view, y).  Nothing of the law is here: drt_image.h, drt_image_loss.h
// and drt_shade.h are used as they are.
//   The k listed views (slots 0 .. k - 1, repeats allowed) are stacked into a tall image of k * H rows; row r is row r % H of slot r / H.
//   A slot's view id comes from the call's id list, a kernel argument BY VALUE (ImageViewIds); the id selects a row of the capture's view
//   table in device memory (ImageViewRow: camera and screen).
// Plain C++ like the other law headers, so that tests/hostsim/image_views.cpp runs the mapping on the host.
#pragma once
#include "drt_image.h"

namespace drt {

constexpr int kImageViewsMax = 16;         // views of one call

// One view of a capture: what image_call_check unpacks of camera21 and screen9.
struct ImageViewRow {
    ImageCam cam;
    ImageScreen sc;
};
static_assert(sizeof(ImageViewRow) == 240, "a table row is 21 + 9 doubles");

// The id list of one call: k slots of `height` rows each; id[j] for j >= k is 0.
struct ImageViewIds {
    int height, k;
    int id[kImageViewsMax];
};

// id[slot] without indexing the argument array by a per-lane value (a runtime-indexed array goes to scratch): an unrolled select over
// the at most 16 entries.  slot outside [0, 16) gives id[0].
DRT_HD int image_views_id(const ImageViewIds& v, int slot) {
    int id = v.id[0];
#pragma unroll
    for (int j = 1; j < kImageViewsMax; ++j) id = slot == j ? v.id[j] : id;
    return id;
}

// Row r of the tall image, 0 <= r < k * height -> its slot, the slot's view id and the row y within that view.
DRT_HD void image_views_row(const ImageViewIds& v, int r, int& slot, int& view, int& y) {
    slot = r / v.height;
    y = r - slot * v.height;
    view = image_views_id(v, slot);
}

}  // namespace drt
