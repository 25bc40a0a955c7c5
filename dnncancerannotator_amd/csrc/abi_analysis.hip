// abi_analysis.hip -- the C ABI of everything that analyses probabilities (include/dnnca.h): test-time augmentation, pixel and region
// confusion, the composite, lesion tables (plain, linked, with spread, matched), boundary distances, spread by outcome, calibration,
// temperature scaling and the signed distance map of label planes.  The kernels and their host drivers are in kernels_tta.hip, kernels_region.hip (region.h) and
// kernels_calib.hip (calib.h); what is here validates, resolves which planes are meant, stages them and calls the driver.
#include "abi.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "bootstrap.h"
#include "boundary.h"
#include "calib.h"
#include "detect.h"
#include "kernels.h"
#include "refine.h"
#include "region.h"
#include "topk.h"

using namespace dnnca;

extern "C" {

// ---- test-time augmentation (kernels_tta.hip) ---------------------------------------------------------------------------------
// the views of a mask in ascending order; 0 with the error set when the mask or a transposed view on h x w is refused
static int tta_views_of(unsigned views, int h, int w, int* ks) {
    if (views < 1u || views > 255u) { set_error("tta: views mask %u outside 1..255", views); return 0; }
    if ((views & 0xF0u) && h != w) { set_error("tta: a transposed view (mask 0x%02X) needs a square plane, not %d x %d", views, h, w); return 0; }
    int n = 0;
    for (int k = 0; k < 8; ++k)
        if (views >> k & 1u) ks[n++] = k;
    return n;
}

static void tta_launch_view_in(Model* M, const float* src, float* dst, int B, int H, int W, int C, int k) {
    const double nx = (double)B * H * W * C;
    LAUNCH(M, "tta_view_in", 8.0 * nx, 0.0, g_tta_view_in(M->stream, src, dst, B, H, W, C, k));
}

// where the views of one call go: the mean into prob; with spread != nullptr also the spread, over the three planes of running
// moments mom (`plane` floats apart)
struct TtaTarget { float *prob, *spread, *mom; size_t plane; int B, H, W; bool is_logits; };

// view k, the pos-th of n, mapped back from src and taken into the target
static void tta_launch_view(Model* M, const TtaTarget& t, const float* src, int k, int pos, int n) {
    const double npix = (double)t.B * t.H * t.W;
    if (!t.spread) {
        LAUNCH(M, "tta_accumulate", (pos ? 12.0 : 8.0) * npix, (t.is_logits ? 5.0 : 1.0) * npix,
               g_tta_accumulate(M->stream, src, t.prob, t.B, t.H, t.W, k, t.is_logits, pos == 0, pos == n - 1, n));
        return;
    }
    // floats moved per pixel: the view in; p0 out (view 0) or in; the two sums in (from view 2 on) and out (up to the last but one);
    // the running sum in (from view 1 on) and out; the spread out (last view)
    const bool last = pos == n - 1;
    const double moved = 1 + (last && !pos ? 0 : 1) + (pos > 1 ? 2 : 0) + (pos && !last ? 2 : 0) + (pos ? 1 : 0) + 1 + (last ? 1 : 0);
    LAUNCH(M, "tta_moments", 4.0 * moved * npix, (t.is_logits ? 11.0 : 7.0) * npix,
           g_tta_moments(M->stream, src, t.prob, t.mom, t.spread, t.plane, t.B, t.H, t.W, k, t.is_logits, pos, n));
}

// the buffers of the stand-alone entries: n_in floats in, n_out floats out, one allocation
static int tta_io_buffers(Model* M, size_t n_in, size_t n_out, float** in, float** out) {
    if (n_in + n_out > M->tta_io_n) {
        if (M->tta_io) HIP_TRY(hipFree(M->tta_io));
        M->tta_io = nullptr;
        M->tta_io_n = 0;
        HIP_TRY(hipMalloc((void**)&M->tta_io, (n_in + n_out) * 4));
        M->tta_io_n = n_in + n_out;
    }
    *in = M->tta_io;
    *out = M->tta_io + n_in;
    return DNNCA_OK;
}

// the launch grids carry the rows and the slices in their y and z dimensions
static int tta_check_plane(int batch, int h, int w, int c) {
    if (batch < 1 || h < 1 || w < 1 || c < 1 || h > 65535 || batch > 65535 || (int64_t)w * c > INT32_MAX) {
        set_error("tta: bad plane %d x %d x %d x %d (at most 65535 slices and rows, w * c below 2^31)", batch, h, w, c);
        return DNNCA_EINVAL;
    }
    return DNNCA_OK;
}

// what dnnca_forward_tta*, and dnnca_forward_ensemble for every member, do before their first forward: validate, allocate what the
// views (and, with_spread, their spread) need, stage the batch.  ks receives the views in ascending order; returns their number in *n
static int tta_prepare(Model* M, const float* x_nhwc, int batch, unsigned views, bool with_spread, int* ks, int* n) {
    const int H = M->desc.height, W = M->desc.width, C = M->desc.in_channels;
    *n = tta_views_of(views, H, W, ks);
    if (!*n) return DNNCA_EINVAL;
    if (!x_nhwc) { set_error("tta: null x"); return DNNCA_EINVAL; }
    if (M->outH != H || M->outW != W) {
        set_error("tta: the output (%d x %d) differs from the input (%d x %d)", M->outH, M->outW, H, W);
        return DNNCA_EINVAL;
    }
    DN_TRY(check_batch(M, batch));
    DN_TRY(tta_check_plane(batch, H, W, C));
    const size_t plane = (size_t)M->desc.max_batch * H * W;
    if (!M->tta_view && views != 1u) DN_TRY(M->alloc((void**)&M->tta_view, plane * C * 4));
    if (with_spread && !M->tta_spread) DN_TRY(M->alloc((void**)&M->tta_spread, plane * 4));
    if (with_spread && !M->tta_mom) DN_TRY(M->alloc((void**)&M->tta_mom, 3 * plane * 4));
    return stage_inputs(M, batch, x_nhwc, nullptr, false);
}

// one inference forward per view of the staged batch with the weights that are in place, the mean in M->prob and, with_spread, the
// spread in M->tta_spread
static int tta_body(Model* M, int batch, const int* ks, int n, bool with_spread) {
    const int H = M->desc.height, W = M->desc.width, C = M->desc.in_channels;
    const size_t plane = (size_t)M->desc.max_batch * H * W;
    const TtaTarget t = {M->prob, with_spread ? M->tta_spread : nullptr, M->tta_mom, plane, batch, H, W, true};
    for (int i = 0; i < n; ++i) {
        const float* x = M->x_stage;                      // view 0 forwards from the staged batch itself
        if (ks[i]) {
            tta_launch_view_in(M, M->x_stage, M->tta_view, batch, H, W, C, ks[i]);
            x = M->tta_view;
        }
        DN_TRY(M->forward(x, batch, false));
        tta_launch_view(M, t, M->logits, ks[i], i, n);
    }
    return DNNCA_OK;
}

// dnnca_forward_tta and, with_spread, dnnca_forward_tta_spread up to their read-back
static int tta_forward(Model* M, const float* x_nhwc, int batch, unsigned views, bool with_spread) {
    int ks[8], n = 0;
    DN_TRY(tta_prepare(M, x_nhwc, batch, views, with_spread, ks, &n));
    return tta_body(M, batch, ks, n, with_spread);
}

int dnnca_forward_tta(void* model, const float* x_nhwc, int batch, unsigned views, float* prob_out) {
    MODEL(model);
    DN_TRY(tta_forward(M, x_nhwc, batch, views, false));
    if (prob_out) {
        HIP_TRY(hipMemcpyAsync(prob_out, M->prob, (size_t)batch * M->outH * M->outW * 4, hipMemcpyDeviceToHost, M->stream));
        HIP_TRY(hipStreamSynchronize(M->stream));
        return M->flush_profile();
    }
    return DNNCA_OK;
}

int dnnca_forward_tta_spread(void* model, const float* x_nhwc, int batch, unsigned views, float* prob_out, float* spread_out) {
    MODEL(model);
    DN_TRY(tta_forward(M, x_nhwc, batch, views, true));
    M->tta_spread_valid = true;
    M->tta_spread_batch = batch;
    M->members.spread_valid = false;
    const size_t npix = (size_t)batch * M->outH * M->outW;
    if (prob_out) HIP_TRY(hipMemcpyAsync(prob_out, M->prob, npix * 4, hipMemcpyDeviceToHost, M->stream));
    if (spread_out) HIP_TRY(hipMemcpyAsync(spread_out, M->tta_spread, npix * 4, hipMemcpyDeviceToHost, M->stream));
    if (prob_out || spread_out) {
        HIP_TRY(hipStreamSynchronize(M->stream));
        return M->flush_profile();
    }
    return DNNCA_OK;
}

int dnnca_tta_view_of(void* model, const float* src, int batch, int h, int w, int c, int view, float* dst) {
    MODEL(model);
    if (!src || !dst) { set_error("tta: null buffer"); return DNNCA_EINVAL; }
    if (view < 0 || view > 7) { set_error("tta: view %d outside 0..7", view); return DNNCA_EINVAL; }
    int ks[8];
    if (!tta_views_of(1u << view, h, w, ks)) return DNNCA_EINVAL;
    DN_TRY(check_batch(M, batch));
    DN_TRY(tta_check_plane(batch, h, w, c));
    const size_t nx = (size_t)batch * h * w * c;
    float *in = nullptr, *out = nullptr;
    DN_TRY(tta_io_buffers(M, nx, nx, &in, &out));
    HIP_TRY(hipMemcpyAsync(in, src, nx * 4, hipMemcpyHostToDevice, M->stream));
    tta_launch_view_in(M, in, out, batch, h, w, c, view);
    HIP_TRY(hipMemcpyAsync(dst, out, nx * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return M->flush_profile();
}

// dnnca_tta_mean_of and, with spread_out, dnnca_tta_spread_of: the views of host values, none of the model's planes touched
static int tta_of(void* model, const float* vals, int batch, int h, int w, unsigned views, int is_logits, float* prob_out,
                  float* spread_out) {
    MODEL(model);
    int ks[8];
    const int n = tta_views_of(views, h, w, ks);
    if (!n) return DNNCA_EINVAL;
    if (!vals || !prob_out) { set_error("tta: null buffer"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    DN_TRY(tta_check_plane(batch, h, w, 1));
    const size_t npix = (size_t)batch * h * w;
    float *in = nullptr, *out = nullptr;                 // out: the mean and, with spread_out, the spread, then the three planes of moments
    DN_TRY(tta_io_buffers(M, npix * n, spread_out ? npix * 5 : npix, &in, &out));
    HIP_TRY(hipMemcpyAsync(in, vals, npix * n * 4, hipMemcpyHostToDevice, M->stream));
    const TtaTarget t = {out, spread_out ? out + npix : nullptr, spread_out ? out + 2 * npix : nullptr, npix, batch, h, w, is_logits != 0};
    for (int i = 0; i < n; ++i) tta_launch_view(M, t, in + npix * i, ks[i], i, n);
    HIP_TRY(hipMemcpyAsync(prob_out, out, npix * 4, hipMemcpyDeviceToHost, M->stream));
    if (spread_out) HIP_TRY(hipMemcpyAsync(spread_out, out + npix, npix * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return M->flush_profile();
}

int dnnca_tta_mean_of(void* model, const float* vals, int batch, int h, int w, unsigned views, int is_logits, float* prob_out) {
    return tta_of(model, vals, batch, h, w, views, is_logits, prob_out, nullptr);
}

int dnnca_tta_spread_of(void* model, const float* vals, int batch, int h, int w, unsigned views, int is_logits, float* prob_out,
                        float* spread_out) {
    if (!spread_out) { set_error("tta: null buffer"); return DNNCA_EINVAL; }
    return tta_of(model, vals, batch, h, w, views, is_logits, prob_out, spread_out);
}

static const char* kSpreadState = "dnnca_forward_tta_spread makes it valid, until the next call that rewrites the probabilities";

// the model's own spread plane for `batch` slices, or DNNCA_ESTATE
static int tta_spread_plane(Model* M, int batch, const char* who) {
    if (!M->tta_spread_valid) { set_error("%s: the model's spread plane is not valid (%s)", who, kSpreadState); return DNNCA_ESTATE; }
    if (batch > M->tta_spread_batch) {
        set_error("%s: %d slices asked for, the model's spread plane holds %d (%s)", who, batch, M->tta_spread_batch, kSpreadState);
        return DNNCA_ESTATE;
    }
    return DNNCA_OK;
}

int dnnca_get_tta_spread(void* model, int batch, float* out) {
    MODEL(model);
    if (!out) { set_error("tta: null buffer"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    DN_TRY(tta_spread_plane(M, batch, "dnnca_get_tta_spread"));
    HIP_TRY(hipMemcpyAsync(out, M->tta_spread, (size_t)batch * M->outH * M->outW * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

// ---- ensembles (kernels_ensemble.hip) ------------------------------------------------------------------------------------------
// member `pos` of n joins: floats moved per pixel, as tta_launch_view counts them.  Without between_out: the mean in, es in (from
// member 1 on), es or the mean out.  With it also: the within spread in (when there is one); e0 out (member 0) or in; sum d and
// sum d^2 in (from member 2 on) and out (members 1 up to the last but one); sum s^2 in (from member 1 on) and out (up to the last
// but one); between, within and total out (last member)
static void ens_launch_join(Model* M, size_t npix, const float* mean_in, const float* within_in, float* run, size_t pitch, int pos, int n,
                            float* mean_out, float* between_out, float* within_out, float* total_out) {
    const bool last = pos == n - 1;
    double moved = 1 + (pos ? 1 : 0) + 1;
    if (between_out)
        moved += (within_in ? 1 : 0) + (last && !pos ? 0 : 1) + (pos > 1 ? 2 : 0) + (pos && !last ? 2 : 0) + (pos ? 1 : 0) + (last ? 3 : 1);
    LAUNCH(M, "ens_join", 4.0 * moved * (double)npix, (between_out ? 12.0 : 2.0) * (double)npix,
           g_ens_join(M->stream, npix, mean_in, within_in, run, pitch, pos, n, mean_out, between_out, within_out, total_out));
}

static constexpr int kEnsPlanes = 7;      // es, e0, sum d, sum d^2, sum s^2, between, within (Model::members)

static int member_check(Model* M, int m, const char* who) {
    if (m < 0 || m >= M->members.n) { set_error("%s: member %d outside 0..%d (dnnca_model_set_members)", who, m, M->members.n - 1); return DNNCA_EINVAL; }
    return DNNCA_OK;
}
static float* member_slot(Model* M, int m) { return M->members.w + (size_t)m * (size_t)(M->nT + M->nS); }

int dnnca_model_set_members(void* model, int n) {
    MODEL(model);
    if (n < 0 || n > DNNCA_MAX_MEMBERS) { set_error("dnnca_model_set_members: %d members outside 0..%d", n, DNNCA_MAX_MEMBERS); return DNNCA_EINVAL; }
    HIP_TRY(hipStreamSynchronize(M->stream));
    if (M->members.w) HIP_TRY(hipFree(M->members.w));
    M->members.w = nullptr;
    M->members.n = 0;
    M->members.stored = 0;
    if (n == 0) {
        if (M->members.planes) HIP_TRY(hipFree(M->members.planes));
        M->members.planes = nullptr;
        if (M->members.spread_valid) M->tta_spread_valid = false;      // the two components are gone: so is the total's claim to them
        M->members.spread_valid = false;
        return DNNCA_OK;
    }
    HIP_TRY(hipMalloc((void**)&M->members.w, (size_t)(n + 1) * (size_t)(M->nT + M->nS) * 4));
    M->members.n = n;
    return DNNCA_OK;
}

int dnnca_member_store(void* model, int m, const float* params, int64_t nT, const float* state, int64_t nS) {
    MODEL(model);
    DN_TRY(member_check(M, m, "dnnca_member_store"));
    if (nT != M->nT || nS != M->nS) {
        set_error("dnnca_member_store: vectors of %lld and %lld floats, the model has %lld and %lld", (long long)nT, (long long)nS,
                  (long long)M->nT, (long long)M->nS);
        return DNNCA_EINVAL;
    }
    if (!params || (!state && nS)) { set_error("dnnca_member_store: null vector"); return DNNCA_EINVAL; }
    float* slot = member_slot(M, m);
    HIP_TRY(hipMemcpyAsync(slot, params, (size_t)nT * 4, hipMemcpyHostToDevice, M->stream));
    if (nS) HIP_TRY(hipMemcpyAsync(slot + nT, state, (size_t)nS * 4, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    M->members.stored |= 1u << m;
    return DNNCA_OK;
}

int dnnca_member_get(void* model, int m, float* params, float* state) {
    MODEL(model);
    DN_TRY(member_check(M, m, "dnnca_member_get"));
    if (!(M->members.stored >> m & 1u)) { set_error("dnnca_member_get: member %d was never stored", m); return DNNCA_ESTATE; }
    const float* slot = member_slot(M, m);
    if (params) HIP_TRY(hipMemcpyAsync(params, slot, (size_t)M->nT * 4, hipMemcpyDeviceToHost, M->stream));
    if (state && M->nS) HIP_TRY(hipMemcpyAsync(state, slot + M->nT, (size_t)M->nS * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

// (p, state) <- slot `from`, or slot `to` <- (p, state): contents on the model's stream, in order with the forwards around them
static int member_copy(Model* M, int slot, bool into_model) {
    float* w = member_slot(M, slot);
    float *dp = into_model ? M->p : w, *ds = into_model ? M->state : w + M->nT;
    const float *sp = into_model ? w : M->p, *ss = into_model ? w + M->nT : M->state;
    HIP_TRY(hipMemcpyAsync(dp, sp, (size_t)M->nT * 4, hipMemcpyDeviceToDevice, M->stream));
    if (M->nS) HIP_TRY(hipMemcpyAsync(ds, ss, (size_t)M->nS * 4, hipMemcpyDeviceToDevice, M->stream));
    return DNNCA_OK;
}

// the members of dnnca_forward_ensemble, one after the other, while the model's own weights wait in the spare slot
static int ens_members(Model* M, int batch, const int* ks, int nviews, bool with_spread) {
    const int n = M->members.n;
    const size_t pitch = (size_t)M->desc.max_batch * M->outH * M->outW, npix = (size_t)batch * M->outH * M->outW;
    float* run = M->members.planes;
    const bool member_spread = with_spread && nviews > 1;
    for (int m = 0; m < n; ++m) {
        DN_TRY(member_copy(M, m, true));
        DN_TRY(tta_body(M, batch, ks, nviews, member_spread));
        ens_launch_join(M, npix, M->prob, member_spread ? M->tta_spread : nullptr, run, pitch, m, n, M->prob,
                        with_spread ? run + 5 * pitch : nullptr, run + 6 * pitch, M->tta_spread);
    }
    return DNNCA_OK;
}

int dnnca_forward_ensemble(void* model, const float* x_nhwc, int batch, unsigned views, int with_spread, float* prob_out) {
    MODEL(model);
    DN_TRY(M->ema_refuse("dnnca_forward_ensemble"));
    const int n = M->members.n;
    if (n < 1) { set_error("dnnca_forward_ensemble: the model has no members (dnnca_model_set_members)"); return DNNCA_ESTATE; }
    for (int m = 0; m < n; ++m)
        if (!(M->members.stored >> m & 1u)) {
            set_error("dnnca_forward_ensemble: member %d of %d was never stored (dnnca_member_store)", m, n);
            return DNNCA_ESTATE;
        }
    int ks[8], nviews = 0;
    // the spread plane carries the total also where a single view leaves no within-member spread to take
    DN_TRY(tta_prepare(M, x_nhwc, batch, views, with_spread != 0, ks, &nviews));
    if (!M->members.planes) {
        const size_t bytes = (size_t)kEnsPlanes * M->desc.max_batch * M->outH * M->outW * 4;
        HIP_TRY(hipMalloc((void**)&M->members.planes, bytes));
    }
    DN_TRY(member_copy(M, n, false));
    const int rc = ens_members(M, batch, ks, nviews, with_spread != 0);
    DN_TRY(member_copy(M, n, true));           // whatever a member's forward said, the model's own weights are back
    DN_TRY(rc);
    if (with_spread) {
        M->tta_spread_valid = true;
        M->tta_spread_batch = batch;
        M->members.spread_valid = true;
    }
    if (prob_out) {
        HIP_TRY(hipMemcpyAsync(prob_out, M->prob, (size_t)batch * M->outH * M->outW * 4, hipMemcpyDeviceToHost, M->stream));
        HIP_TRY(hipStreamSynchronize(M->stream));
        return M->flush_profile();
    }
    return DNNCA_OK;
}

int dnnca_get_ensemble_spread(void* model, int batch, float* between_out, float* within_out) {
    MODEL(model);
    DN_TRY(check_batch(M, batch));
    DN_TRY(tta_spread_plane(M, batch, "dnnca_get_ensemble_spread"));
    if (!M->members.spread_valid || !M->members.planes) {
        set_error("dnnca_get_ensemble_spread: the model's spread plane is not an ensemble's (dnnca_forward_ensemble with_spread makes it one)");
        return DNNCA_ESTATE;
    }
    const size_t pitch = (size_t)M->desc.max_batch * M->outH * M->outW, npix = (size_t)batch * M->outH * M->outW;
    if (between_out) HIP_TRY(hipMemcpyAsync(between_out, M->members.planes + 5 * pitch, npix * 4, hipMemcpyDeviceToHost, M->stream));
    if (within_out) HIP_TRY(hipMemcpyAsync(within_out, M->members.planes + 6 * pitch, npix * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

int dnnca_ensemble_of(void* model, const float* means, const float* withins, int n, int batch, int h, int w, float* mean_out,
                      float* between_out, float* within_out, float* total_out) {
    MODEL(model);
    if (n < 1 || n > DNNCA_MAX_MEMBERS) { set_error("ensemble: %d members outside 1..%d", n, DNNCA_MAX_MEMBERS); return DNNCA_EINVAL; }
    if (!means || !mean_out) { set_error("ensemble: null buffer"); return DNNCA_EINVAL; }
    const bool spread = between_out != nullptr;
    if ((within_out != nullptr) != spread || (total_out != nullptr) != spread) {
        set_error("ensemble: between_out, within_out and total_out go together");
        return DNNCA_EINVAL;
    }
    DN_TRY(check_batch(M, batch));
    DN_TRY(tta_check_plane(batch, h, w, 1));
    const size_t npix = (size_t)batch * h * w;
    // in: the means, then the within spreads; out: mean, between, within, total, then the five running planes, npix floats apart
    float *in = nullptr, *out = nullptr;
    DN_TRY(tta_io_buffers(M, npix * n * (withins ? 2 : 1), npix * 9, &in, &out));
    HIP_TRY(hipMemcpyAsync(in, means, npix * n * 4, hipMemcpyHostToDevice, M->stream));
    if (withins) HIP_TRY(hipMemcpyAsync(in + npix * n, withins, npix * n * 4, hipMemcpyHostToDevice, M->stream));
    for (int m = 0; m < n; ++m)
        ens_launch_join(M, npix, in + npix * m, withins ? in + npix * (n + m) : nullptr, out + 4 * npix, npix, m, n, out,
                        spread ? out + npix : nullptr, out + 2 * npix, out + 3 * npix);
    HIP_TRY(hipMemcpyAsync(mean_out, out, npix * 4, hipMemcpyDeviceToHost, M->stream));
    if (spread) {
        HIP_TRY(hipMemcpyAsync(between_out, out + npix, npix * 4, hipMemcpyDeviceToHost, M->stream));
        HIP_TRY(hipMemcpyAsync(within_out, out + 2 * npix, npix * 4, hipMemcpyDeviceToHost, M->stream));
        HIP_TRY(hipMemcpyAsync(total_out, out + 3 * npix, npix * 4, hipMemcpyDeviceToHost, M->stream));
    }
    HIP_TRY(hipStreamSynchronize(M->stream));
    return M->flush_profile();
}

// ---- plane inputs: the model's own planes or the caller's --------------------------------------------------------------------
// Every analysis entry below takes prob_hw == NULL for the model's own probabilities (h and w both 0, or the model's output size)
// or host planes of `batch` slices of h x w.  plane_resolve says which plane that is, plane_stage puts it on the device.
struct Plane { int h, w; size_t hw, n; };      // hw, n: the pixels of a slice, of all `batch` slices

enum : unsigned {
    kPlaneBelow2G = 1u,                  // h, w >= 1 and h * w below 2^31
    kPlaneGridBatch = 2u,                // at most 65535 slices (they are a grid dimension)
    kPlaneHeld = 4u                      // the model's own planes: no more slices than its last forward left
};

// who: the entry's name in messages.  DNNCA_EINVAL for a batch outside the model's, a size that is not the model's, a plane outside
// `limits`; then, with kPlaneHeld, DNNCA_ESTATE for slices the model does not hold
static int plane_resolve(Model* M, const char* who, const float* prob_hw, int batch, int h, int w, unsigned limits, Plane* out) {
    DN_TRY(check_batch(M, batch));
    if (!prob_hw) {
        if ((h != 0 || w != 0) && (h != M->outH || w != M->outW)) {
            set_error("%s: %d x %d given, the last forward's probabilities are %d x %d", who, h, w, M->outH, M->outW);
            return DNNCA_EINVAL;
        }
        h = M->outH;
        w = M->outW;
    }
    if (((limits & kPlaneBelow2G) && (h < 1 || w < 1 || (int64_t)h * w > INT32_MAX)) || ((limits & kPlaneGridBatch) && batch > 65535)) {
        set_error("%s: bad plane %d x %d x %d", who, batch, h, w);
        return DNNCA_EINVAL;
    }
    if ((limits & kPlaneHeld) && !prob_hw && batch > M->last_batch) {
        set_error("%s: %d slices asked for, the model's probabilities hold %d (the last forward's)", who, batch, M->last_batch);
        return DNNCA_ESTATE;
    }
    *out = {h, w, (size_t)h * w, (size_t)batch * h * w};
    return DNNCA_OK;
}

// the planes of one call: probabilities, the spread of the views, labels (nullptr: the entry has none); out: where a result plane goes
// x: the input channels of dnnca_lesion_table_features, x_n floats (kScratchRegion, beside probabilities alone)
struct Planes { const float *prob, *spread, *y; float* out; const float* x = nullptr; size_t x_n = 0; };

// region_inputs forgets the labels kept for dnnca_render_composite, tta_io_buffers does not: every entry keeps the scratch it had
enum Scratch { kScratchRegion, kScratchTtaIo };

// The host planes of n floats each -> the scratch `which`; returns where the entry reads each plane on the device.  host.prob ==
// nullptr: the model's own probabilities and spread plane, and the result goes where it came from.
//   kScratchRegion  no host plane: nothing is touched.  Else the probabilities into the first buffer of region_inputs, the labels
//                   (or, for an entry without labels, the spread; or the channels host.x) into the second
//   kScratchTtaIo   with host probabilities one allocation for every host plane and the want_out planes of the result, in the order
//                   prob, spread, y, out; with the model's own the labels go to M->y_stage
static int plane_stage(Model* M, Scratch which, size_t n, const Planes& host, int want_out, Planes* dev) {
    float* slot[4] = {nullptr, nullptr, nullptr, nullptr};          // prob, spread, y, out
    const float* src[3] = {host.prob, host.spread, host.y};
    float* x_dev = nullptr;
    if (which == kScratchRegion && (host.prob || host.y)) {
        float *first = nullptr, *second = nullptr;
        DN_TRY(region_inputs(M, std::max(n, host.x_n), &first, &second));
        if (host.prob) slot[0] = first;
        if (host.x) x_dev = second;
        else slot[host.y ? 2 : 1] = second;
    } else if (which == kScratchTtaIo && host.prob) {
        int count = 0;
        for (int i = 0; i < 3; ++i) count += src[i] != nullptr;
        float *base = nullptr, *unused = nullptr;
        DN_TRY(tta_io_buffers(M, (size_t)(count + want_out) * n, 0, &base, &unused));
        for (int i = 0; i < 3; ++i)
            if (src[i]) slot[i] = base, base += n;
        if (want_out) slot[3] = base;
    } else if (host.y) {
        slot[2] = M->y_stage;
    }
    for (int i = 0; i < 3; ++i)
        if (src[i] && slot[i]) HIP_TRY(hipMemcpyAsync(slot[i], src[i], n * 4, hipMemcpyHostToDevice, M->stream));
    if (x_dev) HIP_TRY(hipMemcpyAsync(x_dev, host.x, host.x_n * 4, hipMemcpyHostToDevice, M->stream));
    *dev = {slot[0] ? slot[0] : M->prob, slot[1] ? slot[1] : M->tta_spread, slot[2] ? slot[2] : M->y_stage, slot[3] ? slot[3] : M->prob,
            x_dev ? x_dev : M->x_stage, host.x_n};
    return DNNCA_OK;
}

// ---- one-shot pixel confusion of M->prob against y_stage ---------------------------------------------------------------------
static int confusion_counts(Model* M, size_t npix, const float* thresholds, int n, dnnca_confusion* out) {
    if (M->eval_active) { set_error("dnnca_pixel_confusion* inside dnnca_eval_begin .. dnnca_eval_end (the histogram is in use)"); return DNNCA_ESTATE; }
    DN_TRY(confusion_begin(M, thresholds, n));
    confusion_add(M, npix, M->y_stage);
    return confusion_finish(M, out);
}

int dnnca_pixel_confusion(void* model, const float* y_hw, int batch, const float* thresholds, int n, dnnca_confusion* out) {
    MODEL(model);
    if (n < 1 || n > DNNCA_CONF_MAX_THR || !out || !thresholds || !y_hw) {
        set_error("bad confusion arguments (1..%d thresholds)", DNNCA_CONF_MAX_THR);
        return DNNCA_EINVAL;
    }
    DN_TRY(check_batch(M, batch));
    const size_t npix = (size_t)batch * M->outH * M->outW;
    HIP_TRY(hipMemcpyAsync(M->y_stage, y_hw, npix * 4, hipMemcpyHostToDevice, M->stream));
    return confusion_counts(M, npix, thresholds, n, out);
}

int dnnca_pixel_confusion_of(void* model, const float* prob_hw, const float* y_hw, int64_t n_pixels, const float* thresholds,
                             int n, dnnca_confusion* out) {
    MODEL(model);
    if (n < 1 || n > DNNCA_CONF_MAX_THR || !out || !thresholds || !y_hw || !prob_hw) {
        set_error("bad confusion arguments (1..%d thresholds)", DNNCA_CONF_MAX_THR);
        return DNNCA_EINVAL;
    }
    int64_t cap = (int64_t)M->desc.max_batch * M->outH * M->outW;
    if (n_pixels < 1 || n_pixels > cap) { set_error("n_pixels %lld outside 1..%lld", (long long)n_pixels, (long long)cap); return DNNCA_EINVAL; }
    M->tta_spread_valid = false;
    HIP_TRY(hipMemcpyAsync(M->prob, prob_hw, (size_t)n_pixels * 4, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipMemcpyAsync(M->y_stage, y_hw, (size_t)n_pixels * 4, hipMemcpyHostToDevice, M->stream));
    return confusion_counts(M, (size_t)n_pixels, thresholds, n, out);
}

// ---- region-based metrics (kernels_region.hip) --------------------------------------------------------------------------
static int region_one(Model* M, const float* prob_dev, const float* y_dev, int batch, int h, int w, const dnnca_region_spec* spec,
                      dnnca_region_counts* out) {
    if (M->region_eval) { set_error("dnnca_region_confusion* inside dnnca_eval_region_begin .. dnnca_eval_region_end"); return DNNCA_ESTATE; }
    std::vector<RegionSpecHost> specs(1);
    DN_TRY(region_spec_check(spec, h, w, specs[0]));
    DN_TRY(region_prepare(M, specs, batch, h, w));
    DN_TRY(region_accumulate(M, prob_dev, y_dev, batch, h, w));
    std::vector<std::vector<dnnca_region_counts>> counts;
    DN_TRY(region_read(M, counts));
    std::copy(counts[0].begin(), counts[0].end(), out);
    return DNNCA_OK;
}

int dnnca_region_confusion_of(void* model, const float* prob_hw, const float* y_hw, int batch, int h, int w,
                              const dnnca_region_spec* spec, dnnca_region_counts* out) {
    MODEL(model);
    if (!prob_hw || !y_hw || !spec || !out || batch < 1 || h < 1 || w < 1) { set_error("bad region confusion arguments"); return DNNCA_EINVAL; }
    const size_t n = (size_t)batch * h * w;
    float *p_dev = nullptr, *y_dev = nullptr;
    DN_TRY(region_inputs(M, n, &p_dev, &y_dev));
    HIP_TRY(hipMemcpyAsync(p_dev, prob_hw, n * 4, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipMemcpyAsync(y_dev, y_hw, n * 4, hipMemcpyHostToDevice, M->stream));
    return region_one(M, p_dev, y_dev, batch, h, w, spec, out);
}

int dnnca_region_confusion(void* model, const float* y_hw, int batch, const dnnca_region_spec* spec, dnnca_region_counts* out) {
    MODEL(model);
    if (!y_hw || !spec || !out) { set_error("bad region confusion arguments"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    const size_t n = (size_t)batch * M->outH * M->outW;
    HIP_TRY(hipMemcpyAsync(M->y_stage, y_hw, n * 4, hipMemcpyHostToDevice, M->stream));
    return region_one(M, M->prob, M->y_stage, batch, M->outH, M->outW, spec, out);
}

int dnnca_region_confusion_slices(void* model, const float* prob_hw, const float* y_hw, int batch, const dnnca_region_spec* specs,
                                  int n, dnnca_region_counts* out) {
    MODEL(model);
    if (!y_hw || !specs || !out || n < 1) { set_error("bad region confusion arguments"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    if (M->region_eval) { set_error("dnnca_region_confusion* inside dnnca_eval_region_begin .. dnnca_eval_region_end"); return DNNCA_ESTATE; }
    std::vector<RegionSpecHost> hs(n);
    for (int i = 0; i < n; ++i) DN_TRY(region_spec_check(specs + i, M->outH, M->outW, hs[i]));
    const size_t npix = (size_t)batch * M->outH * M->outW;
    float *p_dev = nullptr, *y_dev = nullptr;
    DN_TRY(region_inputs(M, npix, &p_dev, &y_dev));       // the labels stay there for dnnca_render_composite
    HIP_TRY(hipMemcpyAsync(y_dev, y_hw, npix * 4, hipMemcpyHostToDevice, M->stream));
    if (prob_hw) HIP_TRY(hipMemcpyAsync(p_dev, prob_hw, npix * 4, hipMemcpyHostToDevice, M->stream));
    DN_TRY(region_prepare(M, hs, batch, M->outH, M->outW, batch));
    DN_TRY(region_accumulate(M, prob_hw ? p_dev : M->prob, y_dev, batch, M->outH, M->outW, true));
    DN_TRY(region_read_slices(M, batch, out));
    region_set_label_batch(M, batch);
    return DNNCA_OK;
}

int dnnca_render_composite(void* model, const float* y_hw, int batch, float ratio, int overlay, uint8_t* out, int64_t capacity,
                           int32_t* out_hwc) {
    MODEL(model);
    if (!out_hwc || capacity < 0 || (out && capacity == 0)) { set_error("bad render arguments"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    if (M->outH != M->desc.height || M->outW != M->desc.width) {
        set_error("render: the output (%d x %d) differs from the input (%d x %d)", M->outH, M->outW, M->desc.height, M->desc.width);
        return DNNCA_EINVAL;
    }
    int hwc[3];
    const int H = M->desc.height, W = M->desc.width, C = M->desc.in_channels;
    DN_TRY(region_render(M, nullptr, nullptr, nullptr, batch, H, W, C, ratio, overlay, nullptr, 0, hwc));
    std::copy(hwc, hwc + 3, out_hwc);
    if (!out) return DNNCA_OK;
    const float* lab = y_hw ? nullptr : region_label_of(M, batch);
    if (y_hw) {
        HIP_TRY(hipMemcpyAsync(M->y_stage, y_hw, (size_t)batch * H * W * 4, hipMemcpyHostToDevice, M->stream));
        lab = M->y_stage;
    } else if (!lab) {
        set_error("render: no labels given and none kept from dnnca_region_confusion_slices of %d slices", batch);
        return DNNCA_ESTATE;
    }
    return region_render(M, M->x_stage, lab, M->prob, batch, H, W, C, ratio, overlay, out, (size_t)capacity, hwc);
}

int dnnca_eval_region_begin(void* model, const dnnca_region_spec* specs, int n) {
    MODEL(model);
    if (!M->eval_active) { set_error("dnnca_eval_region_begin outside dnnca_eval_begin .. dnnca_eval_end"); return DNNCA_ESTATE; }
    if (n < 1 || !specs) { set_error("dnnca_eval_region_begin: no specs"); return DNNCA_EINVAL; }
    std::vector<RegionSpecHost> hs(n);
    for (int i = 0; i < n; ++i) DN_TRY(region_spec_check(specs + i, M->outH, M->outW, hs[i]));
    DN_TRY(region_prepare(M, hs, M->desc.max_batch, M->outH, M->outW));
    M->region_eval = true;
    return DNNCA_OK;
}

int dnnca_eval_region_end(void* model, dnnca_region_counts* out) {
    MODEL(model);
    if (!M->region_eval) { set_error("dnnca_eval_region_end without dnnca_eval_region_begin"); return DNNCA_ESTATE; }
    M->region_eval = false;
    if (!out) { set_error("null region counts output"); return DNNCA_EINVAL; }
    std::vector<std::vector<dnnca_region_counts>> counts;
    DN_TRY(region_read(M, counts));
    for (const auto& c : counts) out = std::copy(c.begin(), c.end(), out);
    return DNNCA_OK;
}

// ---- mask refinement of the lesion tables and the boundary distances (kernels_refine.hip) -------------------------------------
int dnnca_model_set_lesion_refine(void* model, const dnnca_lesion_refine* cfg) {
    MODEL(model);
    const dnnca_lesion_refine next = cfg ? *cfg : dnnca_lesion_refine{0.f, 0, 0};
    if (const char* why = refine_invalid(next)) { set_error("lesion refine: %s", why); return DNNCA_EINVAL; }
    // the kept planes of the linked and matched chains remember the configuration that made them (lesion_carry_is): under another
    // one they do not count, so no chain mixes masks made under two rules
    M->refine = next;
    return DNNCA_OK;
}

int dnnca_model_get_lesion_refine(void* model, dnnca_lesion_refine* out) {
    MODEL(model);
    if (!out) { set_error("lesion refine: null output"); return DNNCA_EINVAL; }
    *out = M->refine;
    return DNNCA_OK;
}

// ---- `annotator predict`: the lesion table (kernels_region.hip) ---------------------------------------------------------------
static LesionArgs lesion_args(float threshold, float resize_factor, int filter_size, int min_area, int max_lesions) {
    LesionArgs a;
    a.threshold = threshold, a.rf = resize_factor, a.k = filter_size, a.min_area = min_area, a.max_lesions = max_lesions;
    return a;
}

// hysteresis keeps the region at hysteresis_low around the pixels at `threshold`: a call's threshold lies above a set low one
static int lesion_refine_threshold(Model* M, const char* what, float threshold) {
    if (M->refine.hysteresis_low == 0.f || threshold > M->refine.hysteresis_low) return DNNCA_OK;
    set_error("%s: threshold %g is not above the refinement's hysteresis_low %g (dnnca_model_set_lesion_refine)", what, (double)threshold,
              (double)M->refine.hysteresis_low);
    return DNNCA_EINVAL;
}

// the caller's buffer `what` (have: it was given) must hold per_slice entries for each of `batch` slices
static int lesion_room(const char* what, bool have, int64_t capacity, int64_t per_slice, int batch) {
    if (have && capacity >= batch * per_slice) return DNNCA_OK;
    set_error("lesion table: %lld %s needed (%d slices x %lld), capacity %lld", (long long)(batch * per_slice), what, batch,
              (long long)per_slice, have ? (long long)capacity : 0ll);
    return DNNCA_EINVAL;
}

// the arguments of the three lesion-table entries as the caller gave them: which planes, the table all three fill, and what only
// the linked and only the spread entry have
struct LesionPlanesIn { const float* prob_hw; int batch, h, w; };
struct LesionTableOut { dnnca_lesion_row* rows; int64_t rows_capacity, *n_rows; int32_t* totals; uint8_t* mask; int64_t mask_capacity; int32_t* out_hw; };
struct LesionLinkOut { const uint8_t* continues; dnnca_lesion_link* links; int64_t links_capacity, *n_links; };
struct LesionSpreadOut { const float* spread_hw; dnnca_lesion_spread* srows; dnnca_slice_spread* stotals; };
struct LesionFeatOut {
    const float* x_hwc; int channels, bins, ring;
    dnnca_lesion_shape* shape; dnnca_lesion_intensity *body, *ring_out; uint32_t* hist;
};

// dnnca_lesion_table (link == spread == feat == nullptr), dnnca_lesion_table_linked (link), dnnca_lesion_table_spread (spread) and
// dnnca_lesion_table_features (feat)
static int lesion_call(void* model, const LesionPlanesIn& in, LesionArgs a, const LesionTableOut& o, const LesionLinkOut* link,
                       const LesionSpreadOut* spread, const LesionFeatOut* feat = nullptr) {
    MODEL(model);
    const int batch = in.batch;
    Plane pl;
    DN_TRY(plane_resolve(M, "lesion table", in.prob_hw, batch, in.h, in.w, 0, &pl));
    DN_TRY(lesion_check(a, pl.h, pl.w));
    DN_TRY(lesion_refine_threshold(M, "lesion table", a.threshold));
    if (!o.out_hw) { set_error("lesion table: null out_hw"); return DNNCA_EINVAL; }
    int channels = 0;
    if (feat) {                          // before out_hw: a refusal touches no output
        if ((in.prob_hw == nullptr) != (feat->x_hwc == nullptr)) {
            set_error("lesion features: prob_hw and x_hwc go together (both host planes, or both NULL for the model's own)");
            return DNNCA_EINVAL;
        }
        channels = feat->channels;
        if (!feat->x_hwc && (channels == 0 || channels == M->desc.in_channels)) channels = M->desc.in_channels;
        else if (!feat->x_hwc) { set_error("lesion features: %d channels given, the staged batch has %d", channels, M->desc.in_channels); return DNNCA_EINVAL; }
        DN_TRY(lesion_features_check(a, channels, feat->bins, feat->ring));
        if (o.rows && (!feat->shape || !feat->body || (feat->ring && !feat->ring_out) || (feat->bins && !feat->hist))) {
            set_error("lesion features: null shape / body / ring_out / hist");
            return DNNCA_EINVAL;
        }
    }
    o.out_hw[0] = a.oh;
    o.out_hw[1] = a.ow;
    if (!o.rows) return DNNCA_OK;                 // size query
    if (!o.totals || !o.n_rows) { set_error("lesion table: null totals / n_rows"); return DNNCA_EINVAL; }
    DN_TRY(lesion_room("rows", true, o.rows_capacity, a.cap, batch));
    if (o.mask) DN_TRY(lesion_room("mask bytes", true, o.mask_capacity, (int64_t)a.oh * a.ow, batch));
    if (link) {
        if (!link->continues) { set_error("lesion table: null continues"); return DNNCA_EINVAL; }
        DN_TRY(lesion_room("links", link->links && link->n_links, link->links_capacity, a.links_per_slice(), batch));
        if (link->continues[0] && !lesion_carry_is(M, a.oh, a.ow)) {
            set_error("lesion table: continues[0] is set, but no linked call on planes of %d x %d precedes this one", a.oh, a.ow);
            return DNNCA_EINVAL;
        }
    }
    if (spread) {
        if ((in.prob_hw == nullptr) != (spread->spread_hw == nullptr)) {
            set_error("lesion table: prob_hw and spread_hw go together (both host planes, or both NULL for the model's own)");
            return DNNCA_EINVAL;
        }
        if (!spread->srows || !spread->stotals) { set_error("lesion table: null srows / stotals"); return DNNCA_EINVAL; }
        if (!spread->spread_hw) DN_TRY(tta_spread_plane(M, batch, "dnnca_lesion_table_spread"));
    }
    if (feat && !feat->x_hwc) {
        if (batch > M->last_batch) {
            set_error("lesion features: %d slices asked for, the last forward staged %d", batch, M->last_batch);
            return DNNCA_ESTATE;
        }
        if (M->outH != M->desc.height || M->outW != M->desc.width) {
            set_error("lesion features: the output (%d x %d) differs from the input (%d x %d)", M->outH, M->outW, M->desc.height,
                      M->desc.width);
            return DNNCA_ESTATE;
        }
    }
    Planes host = {in.prob_hw, spread ? spread->spread_hw : nullptr, nullptr, nullptr};
    if (feat && feat->x_hwc) host.x = feat->x_hwc, host.x_n = pl.n * (size_t)channels;
    Planes dev;      // without labels the second buffer of region_inputs carries the spread plane or the channels
    DN_TRY(plane_stage(M, kScratchRegion, pl.n, host, false, &dev));
    const bool want_mask = o.mask != nullptr;
    if (feat)
        return lesion_table_features(M, dev.prob, dev.x, channels, batch, pl.h, pl.w, a, o.rows, o.n_rows, o.totals, o.mask, want_mask,
                                     feat->bins, feat->ring, feat->shape, feat->body, feat->ring_out, feat->hist);
    if (spread)
        return lesion_table_spread(M, dev.prob, dev.spread, batch, pl.h, pl.w, a, o.rows, o.n_rows, o.totals, o.mask, want_mask,
                                   spread->srows, spread->stotals);
    if (link)
        return lesion_table_linked(M, dev.prob, batch, pl.h, pl.w, a, o.rows, o.n_rows, o.totals, o.mask, want_mask, link->continues,
                                   link->links, link->n_links);
    return lesion_table(M, dev.prob, batch, pl.h, pl.w, a, o.rows, o.n_rows, o.totals, o.mask, want_mask);
}

int dnnca_lesion_table(void* model, const float* prob_hw, int batch, int h, int w, float threshold, float resize_factor,
                       int filter_size, int min_area, int max_lesions, dnnca_lesion_row* rows, int64_t rows_capacity,
                       int64_t* n_rows, int32_t* totals, uint8_t* mask, int64_t mask_capacity, int32_t* out_hw) {
    return lesion_call(model, {prob_hw, batch, h, w}, lesion_args(threshold, resize_factor, filter_size, min_area, max_lesions),
                       {rows, rows_capacity, n_rows, totals, mask, mask_capacity, out_hw}, nullptr, nullptr);
}

int dnnca_lesion_table_linked(void* model, const float* prob_hw, int batch, int h, int w, float threshold, float resize_factor,
                              int filter_size, int min_area, int max_lesions, dnnca_lesion_row* rows, int64_t rows_capacity,
                              int64_t* n_rows, int32_t* totals, uint8_t* mask, int64_t mask_capacity, int32_t* out_hw,
                              const uint8_t* continues, dnnca_lesion_link* links, int64_t links_capacity, int64_t* n_links) {
    const LesionLinkOut link = {continues, links, links_capacity, n_links};
    return lesion_call(model, {prob_hw, batch, h, w}, lesion_args(threshold, resize_factor, filter_size, min_area, max_lesions),
                       {rows, rows_capacity, n_rows, totals, mask, mask_capacity, out_hw}, &link, nullptr);
}

int dnnca_lesion_table_spread(void* model, const float* prob_hw, int batch, int h, int w, float threshold, float resize_factor,
                              int filter_size, int min_area, int max_lesions, dnnca_lesion_row* rows, int64_t rows_capacity,
                              int64_t* n_rows, int32_t* totals, uint8_t* mask, int64_t mask_capacity, int32_t* out_hw,
                              const float* spread_hw, dnnca_lesion_spread* srows, dnnca_slice_spread* stotals) {
    const LesionSpreadOut spread = {spread_hw, srows, stotals};
    return lesion_call(model, {prob_hw, batch, h, w}, lesion_args(threshold, resize_factor, filter_size, min_area, max_lesions),
                       {rows, rows_capacity, n_rows, totals, mask, mask_capacity, out_hw}, nullptr, &spread);
}

int dnnca_lesion_table_features(void* model, const float* prob_hw, int batch, int h, int w, float threshold, float resize_factor,
                                int filter_size, int min_area, int max_lesions, dnnca_lesion_row* rows, int64_t rows_capacity,
                                int64_t* n_rows, int32_t* totals, uint8_t* mask, int64_t mask_capacity, int32_t* out_hw,
                                const float* x_hwc, int channels, int bins, int ring, dnnca_lesion_shape* shape,
                                dnnca_lesion_intensity* body, dnnca_lesion_intensity* ring_out, uint32_t* hist) {
    const LesionFeatOut feat = {x_hwc, channels, bins, ring, shape, body, ring_out, hist};
    return lesion_call(model, {prob_hw, batch, h, w}, lesion_args(threshold, resize_factor, filter_size, min_area, max_lesions),
                       {rows, rows_capacity, n_rows, totals, mask, mask_capacity, out_hw}, nullptr, nullptr, &feat);
}

int dnnca_lesion_table_matched(void* model, const float* prob_hw, const float* y_hw, int batch, int h, int w, float threshold,
                               float resize_factor, int filter_size, int min_area, int max_lesions, const uint8_t* continues,
                               dnnca_lesion_plane_out* pred, uint8_t* mask, int64_t mask_capacity, dnnca_lesion_plane_out* truth,
                               dnnca_lesion_pairs_out* pairs, int32_t* out_hw) {
    MODEL(model);
    Plane pl;
    DN_TRY(plane_resolve(M, "lesion table", prob_hw, batch, h, w, 0, &pl));
    LesionArgs a = lesion_args(threshold, resize_factor, filter_size, min_area, max_lesions);
    DN_TRY(lesion_check(a, pl.h, pl.w));
    DN_TRY(lesion_refine_threshold(M, "lesion table", a.threshold));
    if (!out_hw) { set_error("lesion table: null out_hw"); return DNNCA_EINVAL; }
    out_hw[0] = a.oh;
    out_hw[1] = a.ow;
    if (!pred || !pred->rows) return DNNCA_OK;      // size query
    if (!y_hw) { set_error("lesion table: null y_hw (the matched call needs the labels)"); return DNNCA_EINVAL; }
    if (!truth || !pairs) { set_error("lesion table: null truth / pairs"); return DNNCA_EINVAL; }
    if (!pred->totals || !truth->totals) { set_error("lesion table: null totals"); return DNNCA_EINVAL; }
    DN_TRY(lesion_room("rows", true, pred->rows_capacity, a.cap, batch));
    if (mask) DN_TRY(lesion_room("mask bytes", true, mask_capacity, (int64_t)a.oh * a.ow, batch));
    if (!continues) { set_error("lesion table: null continues"); return DNNCA_EINVAL; }
    DN_TRY(lesion_room("links", pred->links != nullptr, pred->links_capacity, a.links_per_slice(), batch));
    DN_TRY(lesion_room("true_rows", truth->rows != nullptr, truth->rows_capacity, a.cap, batch));
    DN_TRY(lesion_room("true_links", truth->links != nullptr, truth->links_capacity, a.links_per_slice(), batch));
    DN_TRY(lesion_room("pairs", pairs->pairs != nullptr, pairs->capacity, a.links_per_slice(), batch));
    if (continues[0] && !lesion_match_carry_is(M, a.oh, a.ow)) {
        set_error("lesion table: continues[0] is set, but no matched call on planes of %d x %d precedes this one", a.oh, a.ow);
        return DNNCA_EINVAL;
    }
    Planes dev;
    DN_TRY(plane_stage(M, kScratchRegion, pl.n, {prob_hw, nullptr, y_hw, nullptr}, false, &dev));
    return lesion_table_matched(M, dev.prob, dev.y, batch, pl.h, pl.w, a, continues, pred, mask, mask != nullptr, truth, pairs);
}

int dnnca_surface_distances(void* model, const float* prob_hw, const float* y_hw, int batch, int h, int w, float threshold,
                            float resize_factor, int filter_size, int min_area, int max_samples, int32_t* counts,
                            dnnca_surface_sample* samples, int64_t capacity, int64_t* n_samples, uint8_t* edges,
                            int64_t edges_capacity, int32_t* out_hw) {
    MODEL(model);
    Plane pl;
    DN_TRY(plane_resolve(M, "surface distances", prob_hw, batch, h, w, 0, &pl));
    LesionArgs a = lesion_args(threshold, resize_factor, filter_size, min_area, LesionArgs().max_lesions);      // not looked at
    DN_TRY(lesion_check(a, pl.h, pl.w));
    DN_TRY(lesion_refine_threshold(M, "surface distances", a.threshold));
    if (a.oh > kSurfaceMaxSide || a.ow > kSurfaceMaxSide) {
        set_error("surface distances: planes of %d x %d exceed %d pixels a side", a.oh, a.ow, kSurfaceMaxSide);
        return DNNCA_EINVAL;
    }
    if (!out_hw) { set_error("surface distances: null out_hw"); return DNNCA_EINVAL; }
    out_hw[0] = a.oh;
    out_hw[1] = a.ow;
    if (!counts) return DNNCA_OK;                 // size query
    if (!y_hw) { set_error("surface distances: null y_hw (the call needs the labels)"); return DNNCA_EINVAL; }
    if (max_samples < 1) { set_error("surface distances: max_samples %d (must be >= 1)", max_samples); return DNNCA_EINVAL; }
    if (!samples || !n_samples) { set_error("surface distances: null samples / n_samples"); return DNNCA_EINVAL; }
    const long long plane = (long long)a.oh * a.ow, need = (long long)batch * 2 * std::min<long long>(max_samples, plane);
    if (capacity < need) {
        set_error("surface distances: %lld samples needed (%d slices x 2 x %lld), capacity %lld", need, batch, need / (2 * batch),
                  (long long)capacity);
        return DNNCA_EINVAL;
    }
    if (edges && edges_capacity < (int64_t)batch * plane) {
        set_error("surface distances: edges of %lld bytes needed, capacity %lld", (long long)batch * plane, (long long)edges_capacity);
        return DNNCA_EINVAL;
    }
    Planes dev;
    DN_TRY(plane_stage(M, kScratchRegion, pl.n, {prob_hw, nullptr, y_hw, nullptr}, false, &dev));
    return surface_distances(M, dev.prob, dev.y, batch, pl.h, pl.w, a, max_samples, counts, samples, n_samples, edges);
}

// ---- the spread of the views per outcome (kernels_region.hip) ----------------------------------------------------------------
int dnnca_spread_by_outcome(void* model, const float* prob_hw, const float* spread_hw, const float* y_hw, int batch, int h, int w,
                            const float* thresholds, int n_thresholds, dnnca_spread_outcome* out) {
    MODEL(model);
    if (!y_hw || !thresholds || !out) { set_error("spread by outcome: null y_hw / thresholds / out"); return DNNCA_EINVAL; }
    if (n_thresholds < 1 || n_thresholds > kRegionMaxThr) {
        set_error("spread by outcome: %d thresholds outside 1..%d", n_thresholds, kRegionMaxThr);
        return DNNCA_EINVAL;
    }
    for (int t = 0; t < n_thresholds; ++t)
        if (thresholds[t] != thresholds[t]) { set_error("spread by outcome: threshold %d is NaN", t); return DNNCA_EINVAL; }
    if ((prob_hw == nullptr) != (spread_hw == nullptr)) {
        set_error("spread by outcome: prob_hw and spread_hw go together (both host planes, or both NULL for the model's own)");
        return DNNCA_EINVAL;
    }
    Plane pl;
    DN_TRY(plane_resolve(M, "spread by outcome", prob_hw, batch, h, w, kPlaneBelow2G | kPlaneGridBatch, &pl));
    if (!prob_hw) DN_TRY(tta_spread_plane(M, batch, "dnnca_spread_by_outcome"));
    Planes dev;
    DN_TRY(plane_stage(M, kScratchTtaIo, pl.n, {prob_hw, spread_hw, y_hw, nullptr}, false, &dev));
    DN_TRY(spread_by_outcome(M, dev.prob, dev.spread, dev.y, batch, pl.hw, thresholds, n_thresholds, out));
    return M->flush_profile();
}

// ---- calibration (kernels_calib.hip) ------------------------------------------------------------------------------------------
static bool calib_temperature_ok(float t) { return t >= kCalibMinT && t <= kCalibMaxT; }      // false for a NaN

int dnnca_calibration(void* model, const float* prob_hw, const float* y_hw, int batch, int h, int w, int n_bins,
                      const float* temperatures, int n_temperatures, dnnca_calib_bin* bins, dnnca_calib_total* totals, double* nll) {
    MODEL(model);
    if (!y_hw || !bins || !totals) { set_error("calibration: null y_hw / bins / totals"); return DNNCA_EINVAL; }
    if (n_bins < 1 || n_bins > kCalibMaxBins) { set_error("calibration: %d bins outside 1..%d", n_bins, kCalibMaxBins); return DNNCA_EINVAL; }
    if (n_temperatures < 0 || n_temperatures > kCalibMaxTemps) {
        set_error("calibration: %d temperatures outside 0..%d", n_temperatures, kCalibMaxTemps);
        return DNNCA_EINVAL;
    }
    if (n_temperatures > 0 && (!temperatures || !nll)) { set_error("calibration: temperatures without their array or without nll"); return DNNCA_EINVAL; }
    for (int t = 0; t < n_temperatures; ++t)
        if (!calib_temperature_ok(temperatures[t])) {
            set_error("calibration: temperature %d is %g (outside [%g, %g])", t, (double)temperatures[t], (double)kCalibMinT, (double)kCalibMaxT);
            return DNNCA_EINVAL;
        }
    Plane pl;
    DN_TRY(plane_resolve(M, "calibration", prob_hw, batch, h, w, kPlaneBelow2G | kPlaneGridBatch | kPlaneHeld, &pl));
    Planes dev;
    DN_TRY(plane_stage(M, kScratchTtaIo, pl.n, {prob_hw, nullptr, y_hw, nullptr}, false, &dev));
    DN_TRY(calibration(M, dev.prob, dev.y, batch, pl.hw, n_bins, temperatures, n_temperatures, bins, totals, nll));
    return M->flush_profile();
}

int dnnca_prob_temperature(void* model, const float* prob_hw, int batch, int h, int w, float temperature, float* out_hw) {
    MODEL(model);
    if (!calib_temperature_ok(temperature)) {
        set_error("temperature %g outside [%g, %g]", (double)temperature, (double)kCalibMinT, (double)kCalibMaxT);
        return DNNCA_EINVAL;
    }
    if (prob_hw && !out_hw) { set_error("temperature: a host plane needs out_hw"); return DNNCA_EINVAL; }
    Plane pl;
    DN_TRY(plane_resolve(M, "temperature", prob_hw, batch, h, w, kPlaneBelow2G | kPlaneHeld, &pl));
    Planes dev;      // a host plane is scaled into a buffer behind it, the model's own in place
    DN_TRY(plane_stage(M, kScratchTtaIo, pl.n, {prob_hw, nullptr, nullptr, nullptr}, true, &dev));
    DN_TRY(prob_temperature(M, dev.prob, dev.out, pl.n, temperature, out_hw));
    return M->flush_profile();
}

// ---- the detection map (kernels_detect.hip) --------------------------------------------------------------------------------------
int dnnca_detection_map(void* model, const float* prob_hw, int batch, int h, int w, const dnnca_detection_cfg* cfg, float* out_hw,
                        dnnca_detection_row* rows, int64_t* n_rows, dnnca_detection_slice* slices) {
    MODEL(model);
    if (!cfg || !rows || !n_rows || !slices) { set_error("detection: null cfg / rows / n_rows / slices"); return DNNCA_EINVAL; }
    DN_TRY(detection_check(*cfg));
    if (prob_hw && !out_hw) { set_error("detection: a host plane needs out_hw"); return DNNCA_EINVAL; }
    Plane pl;
    DN_TRY(plane_resolve(M, "detection", prob_hw, batch, h, w, kPlaneBelow2G | kPlaneGridBatch | kPlaneHeld, &pl));
    Planes dev;      // a host plane's map goes into a buffer behind it, the model's own is replaced in place
    DN_TRY(plane_stage(M, kScratchTtaIo, pl.n, {prob_hw, nullptr, nullptr, nullptr}, true, &dev));
    DN_TRY(detection_map(M, dev.prob, dev.out, batch, pl.h, pl.w, *cfg, out_hw, rows, n_rows, slices));
    return M->flush_profile();
}

// ---- the bootstrap over exams (kernels_bootstrap.hip) ----------------------------------------------------------------------------
int dnnca_bootstrap_sums(void* model, const int32_t* cols, int E, int K, const int32_t* pool, const int32_t* strata, int S, int R,
                         uint64_t seed, int64_t* out, uint16_t* mult_out) {
    MODEL(model);
    if (!cols || !out) { set_error("bootstrap sums: null cols / out"); return DNNCA_EINVAL; }
    if (K < 1 || K > kBootMaxColumns) { set_error("bootstrap sums: %d columns outside 1..%d", K, kBootMaxColumns); return DNNCA_EINVAL; }
    DN_TRY(bootstrap_check_resampling(E, pool, strata, S, R));
    DN_TRY(bootstrap_sums(M, cols, E, K, pool, strata, S, R, seed, out, mult_out));
    return M->flush_profile();
}

int dnnca_bootstrap_detection(void* model, const dnnca_bootstrap_exam* exams, int E, const dnnca_bootstrap_candidate* cands, int N,
                              const int32_t* pool, const int32_t* strata, int S, int R, uint64_t seed,
                              dnnca_bootstrap_detection_row* out, uint16_t* mult_out) {
    MODEL(model);
    if (!out) { set_error("bootstrap detection: null out"); return DNNCA_EINVAL; }
    DN_TRY(bootstrap_check_resampling(E, pool, strata, S, R));
    DN_TRY(bootstrap_check_detection(exams, E, cands, N));
    DN_TRY(bootstrap_detection(M, exams, E, cands, N, pool, strata, S, R, seed, out, mult_out));
    return M->flush_profile();
}

// ---- the signed distance map of label planes (kernels_boundary.hip) ----------------------------------------------------------
int dnnca_signed_distance_of(void* model, const float* y_hw, int batch, int h, int w, float* phi_out, int32_t* d2_out) {
    MODEL(model);
    if (!y_hw || !phi_out) { set_error("signed distance: null y_hw / phi_out"); return DNNCA_EINVAL; }
    Plane pl;
    DN_TRY(plane_resolve(M, "signed distance", y_hw, batch, h, w, kPlaneBelow2G | kPlaneGridBatch, &pl));
    if (pl.h > kSurfaceMaxSide || pl.w > kSurfaceMaxSide) {
        set_error("signed distance: planes of %d x %d exceed %d pixels a side", pl.h, pl.w, kSurfaceMaxSide);
        return DNNCA_EINVAL;
    }
    // the labels travel as the call's one host plane; behind them the map, the squares and the column pass: a scratch of the call's
    // own, no tensor of the model and no map of a step
    Planes dev;
    DN_TRY(plane_stage(M, kScratchTtaIo, pl.n, {y_hw, nullptr, nullptr, nullptr}, 3, &dev));
    float* phi = dev.out;
    int32_t* d2 = reinterpret_cast<int32_t*>(dev.out + pl.n);
    uint32_t* cols = reinterpret_cast<uint32_t*>(dev.out + 2 * pl.n);
    boundary_transform(M, dev.prob, batch, pl.h, pl.w, cols, phi, d2_out ? d2 : nullptr);
    HIP_TRY(hipMemcpyAsync(phi_out, phi, pl.n * 4, hipMemcpyDeviceToHost, M->stream));
    if (d2_out) HIP_TRY(hipMemcpyAsync(d2_out, d2, pl.n * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return M->flush_profile();
}

// ---- the k-th largest value of planes (kernels_topk.hip) -----------------------------------------------------------------------
int dnnca_topk_select_of(void* model, const float* v_hw, int batch, int hw, int k, float* tau_out, int32_t* n_kept_out) {
    MODEL(model);
    if (!v_hw || !tau_out || !n_kept_out) { set_error("top-k select: null v / tau_out / n_kept_out"); return DNNCA_EINVAL; }
    Plane pl;
    DN_TRY(plane_resolve(M, "top-k select", v_hw, batch, 1, hw, kPlaneBelow2G | kPlaneGridBatch, &pl));
    if (hw > (1 << 30)) { set_error("top-k select: planes of %d values exceed 2^30 (the kernels index a plane with an int)", hw); return DNNCA_EINVAL; }
    if (k < 1 || k > hw) { set_error("top-k select: k %d outside [1, %d]", k, hw); return DNNCA_EINVAL; }
    // the planes travel as the call's one host plane; the workspace is the call's own: no plane and no threshold of a step is touched
    Planes dev;
    DN_TRY(plane_stage(M, kScratchTtaIo, pl.n, {v_hw, nullptr, nullptr, nullptr}, 0, &dev));
    if (!M->topk.select_ws) DN_TRY(M->alloc(&M->topk.select_ws, topk_ws_bytes(M->desc.max_batch)));      // (zeroed: empty histograms)
    topk_select(M, batch, hw, k, dev.prob, M->topk.select_ws);
    std::vector<TopkImage> st((size_t)batch);
    HIP_TRY(hipMemcpyAsync(st.data(), M->topk.select_ws, st.size() * sizeof(TopkImage), hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    for (int b = 0; b < batch; ++b) {
        std::memcpy(tau_out + b, &st[b].tau, 4);
        n_kept_out[b] = (int32_t)st[b].n_kept;
    }
    return M->flush_profile();
}

}  // extern "C"
