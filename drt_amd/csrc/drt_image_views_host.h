// drt_image_views_host.h -- the host side of a capture's view table that the two multi-view units share (drt_image_views.hip makes, frees
// and starts it; drt_image_views_env.hip, DESIGN.md 10.10, uses it): the handle behind drt_image_views_t and the start hook of
// image_forward_from under the table.  No kernel is stated here.
#pragma once
#include "drt_image_wave.h"

// The capture's view table behind drt_image_views_t (drt_image_views.hip makes and frees it).
struct drt_image_views {
    drt_scene* scene = nullptr;
    int n_views = 0, height = 0, width = 0;
    ImageViewRow* d_rows = nullptr;
    double* cam21 = nullptr;               // host copies [n_views, 21] / [n_views, 9]: what image_call_check reads of the first listed view
    double* scr9 = nullptr;
    drt_image_views* next = nullptr;       // the scene's list (drt_scene::image_views)
};

// The start hook of image_forward_from under a view table (defined in drt_image_views.hip, which holds k_image_start<ImageViewTable>):
// `src` points to a ViewsStart.
struct ViewsStart {
    ImageViewTable view;
    ImageBand band;
};
void image_start_views(const ImageStartArgs& a, const void* src);
