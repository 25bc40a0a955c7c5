// region.h -- region-based (lesion-level) metrics on the device (kernels_region.hip): the host side of the pipeline that the C ABI
// of abi_analysis.hip drives (dnnca_region_confusion*, dnnca_eval_region_*, the lesion tables, the boundary distances).  The device
// helpers of its connected-component kernels are in ccl_dev.h, which kernels_detect.hip shares.
#pragma once
#include <algorithm>

#include "model.h"

namespace dnnca {

constexpr int kRegionMaxThr = 64;        // thresholds per spec (two 32-bit mask words per pixel)
constexpr int kRegionMaxK = 15;          // morphological filter size
constexpr int kSurfaceMaxSide = 16384;   // boundary distances: analysed planes of up to this many pixels a side (squares in int32)
constexpr unsigned kSurfaceFar = 0x7fffu;   // column distance "none" of surface_cols / boundary_cols: above every real distance

// the bilinear resize of a plane as the kernels take it (kernels_region.hip resize_at; identity: in == out, plain reads)
struct Resize {
    int in_h, in_w, out_h, out_w;
    float sy, sx;                        // in / out as float (TF's CalculateResizeScale), computed on the host
    int identity;
};

// one validated spec: the caller's thresholds (in their order), IoU threshold, resize factor, filter size, and the resized plane
struct RegionSpecHost {
    std::vector<float> thr;
    float iou = 0.3f, rf = 1.f;
    int k = 5;
    int oh = 0, ow = 0;                  // int(fp16(H) * fp16(rf)), int(fp16(W) * fp16(rf))
};

// checks one caller spec against slices of h x w; fills `out` or returns DNNCA_EINVAL with the reason in dnnca_last_error
int region_spec_check(const dnnca_region_spec* s, int h, int w, RegionSpecHost& out);
// uploads the specs' thresholds and zeroes the uint64 accumulators [n_specs][kRegionMaxThr][4]; sizes the workspace for batches of
// up to max_batch slices of h x w.  slices > 0: also zeroes per-slice accumulators [slices][n_specs][kRegionMaxThr][4]
int region_prepare(Model* M, const std::vector<RegionSpecHost>& specs, int max_batch, int h, int w, int slices = 0);
// the counts of `batch` slices prob [batch, h, w] / y [batch, h, w] (device) added to the accumulators of every spec (per_slice:
// slice b's counts to its own accumulator instead)
int region_accumulate(Model* M, const float* prob, const float* y, int batch, int h, int w, bool per_slice = false);
// synchronises and reads the per-slice accumulators: batch x sum(n_thresholds) entries, slice after slice, spec after spec
int region_read_slices(Model* M, int batch, dnnca_region_counts* out);
// synchronises and reads the accumulators: counts[i] = spec i's T entries in the caller's threshold order
int region_read(Model* M, std::vector<std::vector<dnnca_region_counts>>& counts);
// device buffers of the caller-supplied slices (dnnca_region_confusion_of, the labels of dnnca_region_confusion_slices), grown on
// demand; the labels kept for dnnca_render_composite are forgotten
int region_inputs(Model* M, size_t n, float** prob_dev, float** y_dev);
// the label buffer holds the labels of `batch` slices that dnnca_render_composite may reuse; region_label_of(M, batch): that
// buffer if it holds `batch` slices' labels, else nullptr
void region_set_label_batch(Model* M, int batch);
const float* region_label_of(Model* M, int batch);
// the Visualizer's composite of `batch` slices (device x [batch, h, w, c], lab / prob [batch, h, w]) into host `out` (uint8
// [batch, oh, ow, overlay ? 3 : 1]); out_hwc = (oh, ow, channels).  out == nullptr: size query only
int region_render(Model* M, const float* x, const float* lab, const float* prob, int batch, int h, int w, int c, float ratio,
                  int overlay, unsigned char* out, size_t capacity, int* out_hwc);
// ---- the lesion table of dnnca_lesion_table (`annotator predict`): the prediction plane alone through prep (T = 1), open, ccl and
// sizes, then lesion_scan / lesion_stats / lesion_mask, chunked like region_accumulate in the same workspace
struct LesionArgs {
    float threshold = 0.5f, rf = 1.f;
    int k = 5, min_area = 0, max_lesions = 256;
    int oh = 0, ow = 0, cap = 0;         // filled by lesion_check: the analysed plane, rows per slice min(max_lesions, (oh ow + 1) / 2)
    // links into one slice: distinct (row_prev, row) pairs, at most cap^2 and at most ceil(oh ow / 2) (kernels_region.hip, lesion_link);
    // the (row_true, row) pairs of one slice have the same bound (lesion_match)
    int64_t links_per_slice() const { return std::min<int64_t>((int64_t)cap * cap, ((int64_t)oh * ow + 1) / 2); }
};
// checks the caller's arguments against slices of h x w and fills oh / ow / cap; DNNCA_EINVAL with the reason otherwise
int lesion_check(LesionArgs& a, int h, int w);
// prob: device [batch, h, w].  rows (host, batch * a.cap entries at least) receives *n_rows rows, totals (host [batch]) the kept
// components per slice, mask (host uint8 [batch, oh, ow], or nullptr: no mask launch) the cleaned mask.  Synchronises.  In a dry
// run (M->dry) the host outputs are not touched and want_mask stands for `mask != nullptr`
int lesion_table(Model* M, const float* prob, int batch, int h, int w, const LesionArgs& a, dnnca_lesion_row* rows, int64_t* n_rows,
                 int32_t* totals, uint8_t* mask, bool want_mask);
// lesion_table plus the spread of the test-time-augmentation views under it (dnnca_lesion_table_spread): the same chunk loop with the
// same launches and, per chunk, lesion_spread on `spread` (device [batch, h, w], read through the resize of the probabilities).
// srows (host, as many records as rows) receives one record per row of `rows`, stotals (host [batch]) every slice's total
int lesion_table_spread(Model* M, const float* prob, const float* spread, int batch, int h, int w, const LesionArgs& a,
                        dnnca_lesion_row* rows, int64_t* n_rows, int32_t* totals, uint8_t* mask, bool want_mask,
                        dnnca_lesion_spread* srows, dnnca_slice_spread* stotals);
// lesion_table plus what every numbered lesion looks like in the input channels (dnnca_lesion_table_features): the same chunk loop
// with the same launches and, per chunk, lesion_features and (ring > 0) lesion_ring on x (device [batch, h, w, channels], read
// through the resize of the probabilities).  shape (host, as many records as rows), body / ring_out (channels records per row) and
// hist (channels * bins counts per row) receive the records beside `rows`; ring_out is not touched with ring == 0, hist not with
// bins == 0.  The caller has checked lesion_features_check.  In a dry run none of the host pointers is read
int lesion_features_check(const LesionArgs& a, int channels, int bins, int ring);
int lesion_table_features(Model* M, const float* prob, const float* x, int channels, int batch, int h, int w, const LesionArgs& a,
                          dnnca_lesion_row* rows, int64_t* n_rows, int32_t* totals, uint8_t* mask, bool want_mask, int bins, int ring,
                          dnnca_lesion_shape* shape, dnnca_lesion_intensity* body, dnnca_lesion_intensity* ring_out, uint32_t* hist);
// resize factor, filter size, mask choice, bins and ring of the last lesion_table_features (DNNCA_PLAN_LESION_FEATURES); the defaults
// before any
void lesion_features_last(Model* M, float* rf, int* k, bool* want_mask, int* bins, int* ring);
// pixels and q24 spread sums per outcome class (dnnca_spread_by_outcome) of the device planes prob / spread / y [batch, hw] at
// n_thresholds host thresholds: one spread_outcome launch; out (host) [n_thresholds][batch].  Synchronises
int spread_by_outcome(Model* M, const float* prob, const float* spread, const float* y, int batch, size_t hw, const float* thresholds,
                      int n_thresholds, dnnca_spread_outcome* out);
// lesion_table plus the overlap links between neighbouring slices (dnnca_lesion_table_linked): the same chunk loop with the same
// launches, then lesion_link / lesion_link_emit / lesion_carry per chunk.  continues (host [batch]): slice b follows slice b - 1 of
// its exam; the predecessor of a chunk's first slice is the carry plane, i.e. the last slice of the chunk or of the linked call
// before.  links (host, batch * a.links_per_slice() entries at least) receives *n_links links sorted by (slice, row_prev, row).  The caller
// has checked lesion_carry_is(M, a.oh, a.ow) where continues[0] is set.  In a dry run continues / links / n_links are not read
int lesion_table_linked(Model* M, const float* prob, int batch, int h, int w, const LesionArgs& a, dnnca_lesion_row* rows,
                        int64_t* n_rows, int32_t* totals, uint8_t* mask, bool want_mask, const uint8_t* continues,
                        dnnca_lesion_link* links, int64_t* n_links);
// the carry plane holds the rows of the last slice of a successful lesion_table_linked on planes of oh x ow under the model's
// current mask refinement
bool lesion_carry_is(Model* M, int oh, int ow);
// lesion_table_linked on prob plus the same on the labels y (device [batch, h, w]: label' > 0.5, no opening, no area filter, the
// same cap) plus the pairs of a labelled and a predicted lesion of one slice (dnnca_lesion_table_matched): per chunk the launches
// of lesion_table for either plane, then lesion_match (the three kinds of pairs in one pass), lesion_link_emit over the three
// sets of tables, lesion_match_carry.  pred / truth / pairs: the caller's buffers (checked by the caller) and the counts written
// back; every list sorted as lesion_table_linked sorts its links.  The two carry planes are this call's own: the caller has
// checked lesion_match_carry_is(M, a.oh, a.ow) where continues[0] is set.  In a dry run none of the host pointers is read
int lesion_table_matched(Model* M, const float* prob, const float* y, int batch, int h, int w, const LesionArgs& a,
                         const uint8_t* continues, dnnca_lesion_plane_out* pred, uint8_t* mask, bool want_mask,
                         dnnca_lesion_plane_out* truth, dnnca_lesion_pairs_out* pairs);
bool lesion_match_carry_is(Model* M, int oh, int ow);
// resize factor, filter size and mask choice of the last lesion_table_matched (DNNCA_PLAN_LESION_MATCHED); the defaults before any
void lesion_match_last(Model* M, float* rf, int* k, bool* want_mask);
// resize factor, filter size and mask choice of the last lesion_table / lesion_table_linked (DNNCA_PLAN_LESION,
// DNNCA_PLAN_LESION_LINKED); the defaults before any
void lesion_last(Model* M, float* rf, int* k, bool* want_mask);
// ---- the boundary distances of dnnca_surface_distances: the prediction plane through prep, open, ccl and sizes as lesion_table puts
// it (a.max_lesions is not looked at), the label plane through prep alone (label' > 0.5), then surface_edges / surface_cols /
// surface_sample per chunk, in the same workspace.  prob, y: device [batch, h, w].  counts (host [batch][5]), samples (host,
// batch * 2 * min(max_samples, a.oh * a.ow) entries at least, sorted by (slice, side, pixel)) and *n_samples are written; edges
// (host uint8 [batch, oh, ow]) where it is not nullptr.  No carry plane is read or written.  Synchronises.  In a dry run none of the
// host pointers is touched
int surface_distances(Model* M, const float* prob, const float* y, int batch, int h, int w, const LesionArgs& a, int max_samples,
                      int32_t* counts, dnnca_surface_sample* samples, int64_t* n_samples, uint8_t* edges);
// resize factor and filter size of the last surface_distances (DNNCA_PLAN_SURFACE); the defaults before any
void surface_last(Model* M, float* rf, int* k);
void region_release(Model* M);

}  // namespace dnnca
