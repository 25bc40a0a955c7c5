// model.hip -- plan builder (Keras build order of the reference's layers), step orchestration and the C ABI.
//
// Reference structure followed (annotator/models/tf_models): components.py:16-81 Downsample, :84-166 Upsample,
// :169-247 Encoder, :250-320 Decoder; unet.py:19-88 UNet, :91-191 MulmoUNet, :194-300 annotators.
#include "abi.h"

#include <rccl/rccl.h>
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "fast.h"
#include "kernels.h"
#include "optim.h"
#include "accum.h"
#include "region.h"
#include "region_loss.h"
#include "boundary.h"
#include "detect.h"
#include "topk.h"
#include "sens.h"
#include "attr.h"

namespace dnnca {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

enum { kScalars = 8 };

// The one place the small-channel step reads its environment (model.h StepSwitches; Model::build stores the answer in Model::sw).
StepSwitches step_switches() {
    auto on = [](const char* name) { return getenv(name) != nullptr; };
    auto num = [](const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; };
    auto str = [](const char* name) { return std::string(getenv(name) ? getenv(name) : ""); };
    StepSwitches s;
    s.no_fused = on("DNNCA_NO_FUSED");
    s.no_fused_bwd = on("DNNCA_NO_FUSED_BWD");
    s.no_first3 = on("DNNCA_NO_FIRST3");
    s.no_first3f = on("DNNCA_NO_FIRST3F");
    s.no_up3f = on("DNNCA_NO_UP3F");
    s.no_tail3 = on("DNNCA_NO_TAIL3");
    s.no_tcf = on("DNNCA_NO_TCF");
    s.no_tcm = on("DNNCA_NO_TCM");
    s.no_tconv_ride = on("DNNCA_NO_TCONV_RIDE");
    s.no_prep_ride = on("DNNCA_NO_PREP_RIDE");
    s.no_fold_adam = on("DNNCA_NO_FOLD_ADAM");
    s.no_fold_acc = on("DNNCA_NO_FOLD_ACC");
    s.no_pool_fold = on("DNNCA_NO_POOL_FOLD");
    s.no_bwd3v = on("DNNCA_NO_BWD3V");
    s.no_vw = on("DNNCA_NO_VW");
    s.no_head_in_conv = on("DNNCA_NO_HEAD_IN_CONV");
    s.no_label_fusion = on("DNNCA_NO_LABEL_FUSION");
    s.no_wg_stream = on("DNNCA_NO_WG_STREAM");
    s.pgbwd_old = on("DNNCA_PGBWD_OLD");
    s.fz_up2 = on("DNNCA_FZ_UP2");
    s.fz_all = on("DNNCA_FZ_ALL");
    s.lockstep = on("DNNCA_LOCKSTEP");
    s.force_rccl = on("DNNCA_FORCE_RCCL");
    s.no_join = on("DNNCA_NO_JOIN");
    s.fz_only = str("DNNCA_FZ_ONLY");
    s.fzb_only = str("DNNCA_FZB_ONLY");
    if (sscanf(str("DNNCA_STAMPS").c_str(), "%d,%d,%d", &s.stamp_c, &s.stamp_ns, &s.stamp_co) != 3) s.stamp_c = s.stamp_ns = s.stamp_co = 0;
    s.stamps_pf = on("DNNCA_STAMPS_PF");
    s.dbg = num("DNNCA_DBG", 0);
    s.fzb_dbg = num("DNNCA_FZB_DBG", 0);
    s.f3f_abl = num("DNNCA_F3F_ABL", 0);
    s.abl = num("DNNCA_ABL", 0);
    s.tail3_variant = num("DNNCA_TAIL3_VARIANT", 0);
    s.nblocks = std::max(num("DNNCA_NBLOCKS", 0), 0);
    s.pg_maxocc = num("DNNCA_PG_MAXOCC", 3);
    s.tail3_slots = num("DNNCA_TAIL3_SLOTS", 2048);
    s.tail3_lds = num("DNNCA_TAIL3_LDS", 0);
    s.lockstep_maxh = num("DNNCA_LOCKSTEP_MAXH", 128);
    s.wg_prio = num("DNNCA_WG_PRIO", 1);
    if (const char* e = getenv("DNNCA_BUCKET_BYTES")) s.bucket_bytes = std::max((size_t)atol(e), (size_t)4096);
    return s;
}

// train step / its plan dump: the head is to ride in the epilogue of the conv that feeds it (Model::forward decides whether it can).
// Label smoothing blurs the labels in loss_and_backward first: then the head cannot run inside the forward pass.  Nor can it with
// the region loss: a pixel's gradient needs the sums over its whole image (kernels_region_loss.hip).
static bool head_in_conv_requested(const Model* M, const dnnca_loss_cfg& cfg) {
    return !cfg.label_smoothing && !M->region_loss.on && M->merged_launches() && !M->sw.no_head_in_conv;
}

Model::~Model() {
    region_release(this);
    fast_release(this);
    ig_release(this);
    for (void* a : allocs) (void)hipFree(a);
    if (ema.e) (void)hipFree(ema.e);
    if (accum.a) (void)hipFree(accum.a);
    if (opt.table) (void)hipFree(opt.table);
    if (tta_io) (void)hipFree(tta_io);
    if (members.w) (void)hipFree(members.w);
    if (members.planes) (void)hipFree(members.planes);
    if (calib_ws) (void)hipFree(calib_ws);
    if (detect_ws) (void)hipFree(detect_ws);
    if (boot_ws) (void)hipFree(boot_ws);
    for (auto& r : recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto e : evpool) (void)hipEventDestroy(e);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (comm) ncclCommDestroy(comm);
    if (ev_bucket) (void)hipEventDestroy(ev_bucket);
    if (ev_comm_done) (void)hipEventDestroy(ev_comm_done);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    for (auto& sl : stage) {
        if (sl.uploaded) (void)hipEventDestroy(sl.uploaded);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (out_ring) (void)hipHostFree(out_ring);
    if (tm_pin) (void)hipHostFree(tm_pin);
    for (HostRowRing* r : {&aug_ring, &warp_ring, &warpg_ring, &affine_ring, &intensity_ring}) r->release();
    if (wg_fork) (void)hipEventDestroy(wg_fork);
    if (wg_join) (void)hipEventDestroy(wg_join);
    if (wg_bucket) (void)hipEventDestroy(wg_bucket);
    if (wg_stream) (void)hipStreamDestroy(wg_stream);
    if (stream) (void)hipStreamDestroy(stream);
}

bool Model::wg_side_begin() {
    const bool off = sw.no_wg_stream;
    // full profiles (modes 1, 3) time one launch after the other (the sampled bracket of mode 2 goes where its kernel goes); the
    // dry run launches nothing.  (With a communicator a gradient bucket also waits for the side stream: send_bucket.)
    if (off || dry || prof_mode == 1 || prof_mode == 3) return false;
    if (!wg_stream) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);           // lo: the numerically largest = least urgent
        const int prio = sw.wg_prio == 1 ? lo : (sw.wg_prio == 2 ? hi : 0);
        if (hipStreamCreateWithPriority(&wg_stream, hipStreamNonBlocking, prio) != hipSuccess) { wg_stream = nullptr; return false; }
        if (hipEventCreateWithFlags(&wg_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&wg_join, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&wg_bucket, hipEventDisableTiming) != hipSuccess)
            return false;
    }
    if (!wg_fork || !wg_join || !wg_bucket) return false;
    if (hipEventRecord(wg_fork, stream) != hipSuccess || hipStreamWaitEvent(wg_stream, wg_fork, 0) != hipSuccess) return false;
    step.wg_pending = true;
    stream = wg_stream;
    return true;
}

void Model::wg_side_end(hipStream_t main) { stream = main; }

int Model::wg_side_join() {
    if (!step.wg_pending) return DNNCA_OK;
    step.wg_pending = false;
    HIP_TRY(hipEventRecord(wg_join, wg_stream));
    HIP_TRY(hipStreamWaitEvent(stream, wg_join, 0));
    return DNNCA_OK;
}

int Model::alloc(void** ptr, size_t bytes) {
    if (bytes == 0) bytes = 4;
    HIP_TRY(hipMalloc(ptr, bytes));
    allocs.push_back(*ptr);
    HIP_TRY(hipMemsetAsync(*ptr, 0, bytes, stream));
    return DNNCA_OK;
}

int HostRowRing::upload(Model* M, std::initializer_list<Piece> pieces, size_t extra_dev, size_t min_row) {
    size_t bytes = 0;
    for (const Piece& q : pieces) bytes += q.bytes;
    const size_t row = bytes > min_row ? bytes : min_row;
    if (row + extra_dev > dev_bytes) {
        void* p = nullptr;
        DN_TRY(M->alloc(&p, row + extra_dev));
        dev = (char*)p;
        dev_bytes = row + extra_dev;
    }
    if (row > pin_bytes) {
        HIP_TRY(hipStreamSynchronize(M->stream));         // uploads from the old rows are complete
        if (pin) (void)hipHostFree(pin);
        pin = nullptr;
        pin_bytes = 0;
        HIP_TRY(hipHostMalloc((void**)&pin, row * kAugRing, hipHostMallocDefault));
        pin_bytes = row;
    }
    const int r = k;
    k = (r + 1) % kAugRing;
    if (!ev[r]) HIP_TRY(hipEventCreateWithFlags(&ev[r], hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(ev[r]));
    char* dst = pin + (size_t)r * pin_bytes;
    size_t at = 0;
    for (const Piece& q : pieces) {
        memcpy(dst + at, q.host, q.bytes);
        at += q.bytes;
    }
    HIP_TRY(hipMemcpyAsync(dev, dst, bytes, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipEventRecord(ev[r], M->stream));
    return DNNCA_OK;
}

void HostRowRing::release() {
    if (pin) (void)hipHostFree(pin);
    for (auto e : ev)
        if (e) (void)hipEventDestroy(e);
}

void Model::set_variant(const char* fmt, ...) {
    char buf[64];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    variant = buf;
}

// ---------------------------------------------------------------------------------------------- launch accounting
bool Model::begin(const char* name, double bytes, double flops) {
    if (dry) {
        char line[256];
        snprintf(line, sizeof(line), "%s%s%s\t%.0f\t%.0f\n", name, variant.empty() ? "" : "#", variant.c_str(), bytes, flops);
        plan_text += line;
        variant.clear();
        return false;
    }
    if (prof_mode == 0) return true;
    if (prof_mode == 2 && (focus != name || (prof_period > 1 && iterations % prof_period != 0))) return true;
    int id;
    std::string key = name;
    if (prof_mode == 3 && cur_op) key += "@" + *cur_op;          // per-layer table
    auto it = kid.find(key);
    if (it == kid.end()) {
        id = (int)kstats.size();
        kid[key] = id;
        KStat ks;
        ks.name = key;
        kstats.push_back(ks);
    } else {
        id = it->second;
    }
    KStat& ks = kstats[id];
    ks.bytes += bytes;
    ks.flops += flops;
    ks.launches += 1;
    Rec r;
    r.id = id;
    auto get = [&]() {
        hipEvent_t e = nullptr;
        if (!evpool.empty()) {
            e = evpool.back();
            evpool.pop_back();
        } else {
            (void)hipEventCreate(&e);
        }
        return e;
    };
    r.a = get();
    r.b = get();
    (void)hipEventRecord(r.a, stream);
    recs.push_back(r);
    return true;
}

void Model::end() {
    if (dry || prof_mode == 0 || recs.empty()) return;
    Rec& r = recs.back();
    if (r.b && r.id >= 0) {
        (void)hipEventRecord(r.b, stream);
        r.id = -r.id - 1;   // mark closed
    }
}

int Model::flush_profile() {
    if (recs.empty()) return DNNCA_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    for (auto& r : recs) {
        int id = r.id < 0 ? -r.id - 1 : r.id;
        float ms = 0.f;
        if (r.id < 0 && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) kstats[id].total_ms += ms;
        evpool.push_back(r.a);
        evpool.push_back(r.b);
    }
    recs.clear();
    return DNNCA_OK;
}

// ---------------------------------------------------------------------------------------------- plan
int64_t Model::add_param(const std::string& name, std::initializer_list<int64_t> shape, int trainable) {
    ParamInfo pi;
    pi.name = name;
    pi.ndim = (int)shape.size();
    pi.size = 1;
    int i = 0;
    for (int k = 0; k < 4; ++k) pi.shape[k] = 1;
    for (auto s : shape) {
        pi.shape[i++] = s;
        pi.size *= s;
    }
    pi.trainable = trainable;
    int64_t& n = trainable ? nT : nS;
    pi.offset = n;
    n += pi.size;
    params.push_back(pi);
    return pi.offset;
}

// tensors are allocated immediately (stream-ordered memset) -- simple and the sizes are static
T Model::new_tensor(int H, int W, int C, int* rc) {
    T t;
    size_t n = (size_t)desc.max_batch * H * W * C;
    float *dp = nullptr, *gp = nullptr;
    if (*rc == DNNCA_OK) *rc = alloc((void**)&dp, n * 4);
    if (*rc == DNNCA_OK) *rc = alloc((void**)&gp, n * 4);
    t.d.p = dp; t.d.H = H; t.d.W = W; t.d.C = C; t.d.ps = C;
    t.g = t.d;
    t.g.p = gp;
    return t;
}

int Model::build() {
    sw = step_switches();
    if (desc.arch == DNNCA_ARCH_MULTIRES) return build_multires();
    const dnnca_model_desc& d = desc;
    if (d.arch != DNNCA_ARCH_UNET && d.arch != DNNCA_ARCH_MULMO) { set_error("unknown arch %d", d.arch); return DNNCA_EINVAL; }
    if (d.conv_stride != 1) { set_error("conv_stride %d unsupported (reference configs use 1)", d.conv_stride); return DNNCA_EINVAL; }
    if (d.padding != DNNCA_PAD_SAME) { set_error("padding: valid is unsupported (every reference config uses same; labels could not match the cropped logits in utils/losses.py:34)"); return DNNCA_EINVAL; }
    if (d.kernel_size < 1 || d.kernel_size % 2 == 0) { set_error("kernel_size %d must be odd", d.kernel_size); return DNNCA_EINVAL; }
    if (d.in_channels < 1 || d.n_filters_first < 1 || d.n_downsample < 1 || d.rate < 2 || d.n_conv < 1 || d.max_batch < 1) { set_error("bad model_options"); return DNNCA_EINVAL; }
    if (d.dtype != DNNCA_F32 && d.dtype != DNNCA_BF16) { set_error("unknown dtype"); return DNNCA_EINVAL; }
    int div = 1;
    for (int i = 0; i < d.n_downsample; ++i) div *= d.rate;
    if (d.height % div || d.width % div) { set_error("H, W (%d, %d) must be divisible by rate^n_downsample = %d", d.height, d.width, div); return DNNCA_EINVAL; }
    const bool mulmo = d.arch == DNNCA_ARCH_MULMO;
    const int nenc = mulmo ? d.in_channels : 1;
    if (mulmo && (d.reference_index < 0 || d.reference_index >= nenc)) { set_error("reference_index out of range"); return DNNCA_EINVAL; }
    const int K = d.kernel_size, r = d.rate, L = d.n_downsample;
    const float act = d.leaky_alpha;   // 0 relu, >0 leaky

    auto add_param = [&](const std::string& name, std::initializer_list<int64_t> shape, int trainable) { return this->add_param(name, shape, trainable); };
    int rc = DNNCA_OK;
    auto new_tensor = [&](int H, int W, int C) { return this->new_tensor(H, W, C, &rc); };

    auto add_bn = [&](const std::string& prefix, const T& in, const T& out) {
        Op o;
        o.type = OP_BN;
        o.name = prefix;
        o.inA = in;
        o.out = out;
        int C = in.d.C;
        o.w_off = add_param(prefix + ".gamma", {C}, 1);
        o.b_off = add_param(prefix + ".beta", {C}, 1);
        o.mm_off = add_param(prefix + ".moving_mean", {C}, 0);
        o.mv_off = add_param(prefix + ".moving_variance", {C}, 0);
        if (rc == DNNCA_OK) rc = alloc((void**)&o.coef, (size_t)4 * C * 4);
        if (rc == DNNCA_OK) rc = alloc((void**)&o.ws, (size_t)2 * C * 8);
        ops.push_back(o);
    };
    auto add_conv = [&](const std::string& prefix, const T& inA, const T& inB, const T& out, bool need_din) {
        Op o;
        o.type = OP_CONV;
        o.name = prefix;
        o.inA = inA;
        o.inB = inB;
        o.out = out;
        o.k = K;
        o.alpha = act;
        o.need_din = need_din;
        o.w_off = add_param(prefix + ".kernel", {K, K, inA.d.C + inB.d.C, out.d.C}, 1);
        o.b_off = add_param(prefix + ".bias", {out.d.C}, 1);
        ops.push_back(o);
    };

    xin.d.H = d.height; xin.d.W = d.width; xin.d.C = d.in_channels; xin.d.ps = d.in_channels;
    xin.g = xin.d;
    std::vector<int> filters;
    for (int i = 0, f = d.n_filters_first; i < L; ++i, f *= r) filters.push_back(f);

    T empty;   // C = 0
    std::vector<std::vector<T>> skips(nenc);
    std::vector<T> bottoms(nenc);
    int hb = d.height / div, wb = d.width / div;
    T bottom_cat;
    if (mulmo) bottom_cat = new_tensor(hb, wb, filters[L - 1] * nenc);
    for (int e = 0; e < nenc; ++e) {
        std::string enc = mulmo ? "encoder" + std::to_string(e) : "encoder";
        T cur = mulmo ? tslice(xin, e, 1) : xin;
        bool first = true;
        int H = d.height, W = d.width;
        for (int i = 0; i < L; ++i) {
            std::string p = enc + ".down" + std::to_string(i);
            int f = filters[i];
            for (int j = 0; j < d.n_conv; ++j) {
                T a = new_tensor(H, W, f);
                add_conv(p + ".conv" + std::to_string(j), cur, empty, a, !first);
                first = false;
                cur = a;
                if (d.bn) {
                    T n = new_tensor(H, W, f);
                    add_bn(p + ".bn" + std::to_string(j), cur, n);
                    cur = n;
                }
            }
            skips[e].push_back(cur);
            H /= r;
            W /= r;
            bool last = (i == L - 1);
            T dest = (mulmo && last) ? tslice(bottom_cat, e * f, f) : T();
            T pooled = (d.bn || !(mulmo && last)) ? new_tensor(H, W, f) : dest;
            Op o;
            o.type = OP_POOL;
            o.name = p + ".pool";
            o.inA = cur;
            o.out = pooled;
            o.k = r;
            ops.push_back(o);
            cur = pooled;
            if (d.bn) {
                T n = (mulmo && last) ? dest : new_tensor(H, W, f);
                add_bn(p + ".pool_bn", cur, n);
                cur = n;
            }
        }
        bottoms[e] = cur;
    }
    T cur = mulmo ? bottom_cat : bottoms[0];
    const std::vector<T>& ref = skips[mulmo ? d.reference_index : 0];
    for (int u = 0; u < L; ++u) {
        int i = L - 1 - u;
        int f = filters[i];
        std::string p = "decoder.up" + std::to_string(u);
        int H = cur.d.H * r, W = cur.d.W * r;
        T t = new_tensor(H, W, f);
        Op o;
        o.type = OP_TCONV;
        o.name = p + ".tconv";
        o.inA = cur;
        o.out = t;
        o.k = r;
        o.w_off = add_param(p + ".tconv.kernel", {r, r, f, cur.d.C}, 1);
        o.b_off = add_param(p + ".tconv.bias", {f}, 1);
        ops.push_back(o);
        cur = t;
        if (d.bn) {
            T n = new_tensor(H, W, f);
            add_bn(p + ".tconv_bn", cur, n);
            cur = n;
        }
        T skip = ref[i];
        for (int j = 0; j < d.n_conv; ++j) {
            T a = new_tensor(H, W, f);
            add_conv(p + ".conv" + std::to_string(j), cur, j == 0 ? skip : empty, a, true);
            cur = a;
            if (d.bn) {
                T n = new_tensor(H, W, f);
                add_bn(p + ".bn" + std::to_string(j), cur, n);
                cur = n;
            }
        }
    }
    {
        Op o;
        o.type = OP_HEAD;
        o.name = "head";
        o.inA = cur;
        o.w_off = add_param("head.kernel", {1, 1, cur.d.C, 1}, 1);
        o.b_off = add_param("head.bias", {1}, 1);
        ops.push_back(o);
        outH = cur.d.H;
        outW = cur.d.W;
    }
    if (rc != DNNCA_OK) return rc;

    // backward accumulation flags: the first op (in backward order) to produce a gradient overwrites, later ones add.
    std::map<float*, bool> written;
    for (int i = (int)ops.size() - 1; i >= 0; --i) {
        Op& o = ops[i];
        if (!o.need_din) continue;
        o.accA = written[o.inA.g.p];
        written[o.inA.g.p] = true;
        if (o.type == OP_CONV && o.inB.d.C) {
            o.accB = written[o.inB.g.p];
            written[o.inB.g.p] = true;
        }
    }

    // who reads a BatchNorm's output, and which BatchNorm feeds a conv input (exact tensors only: channel slices do not count)
    for (int b = 0; b < (int)ops.size(); ++b) {
        if (ops[b].type != OP_BN) continue;
        const View& y = ops[b].out.d;
        for (int i = 0; i < (int)ops.size(); ++i) {
            Op& o = ops[i];
            const bool a = o.inA.d.p == y.p && o.inA.d.C == y.C && o.inA.d.ps == y.ps;
            const bool bb = o.type == OP_CONV && o.inB.d.C && o.inB.d.p == y.p && o.inB.d.C == y.C && o.inB.d.ps == y.ps;
            const bool overlap = !a && !bb && ((o.inA.d.p >= y.p && o.inA.d.p < y.p + y.ps) || (o.type == OP_CONV && o.inB.d.C && o.inB.d.p >= y.p && o.inB.d.p < y.p + y.ps));
            if (a || bb || overlap) ops[b].out_readers.push_back(overlap ? -1 : i);          // -1: a reader this analysis does not understand
            if (o.type == OP_CONV && a) o.src_bn[0] = b;
            if (bb) o.src_bn[1] = b;
        }
    }
    // twin structure of the mulmo encoders (model.h: lockstep)
    enc_ops = n_enc = 0;
    if (mulmo && nenc > 1) {
        size_t first_dec = 0;
        while (first_dec < ops.size() && ops[first_dec].name.compare(0, 7, "encoder") == 0) ++first_dec;
        if (first_dec % nenc == 0 && first_dec > 0) {
            const int per = (int)(first_dec / nenc);
            bool same = true;
            for (int e = 1; e < nenc && same; ++e)
                for (int j = 0; j < per && same; ++j) {
                    const Op &a = ops[j], &b = ops[(size_t)e * per + j];
                    same = a.type == b.type && a.k == b.k && a.inA.d.C == b.inA.d.C && a.inA.d.H == b.inA.d.H && a.inA.d.W == b.inA.d.W &&
                           a.inB.d.C == b.inB.d.C && a.out.d.C == b.out.d.C && a.out.d.H == b.out.d.H && a.out.d.W == b.out.d.W;
                }
            if (same) { enc_ops = per; n_enc = nenc; }
        }
    }
    fast_plan_masks(this);
    DN_TRY(ig_plan_half(this));
    return build_buffers();
}

int Model::build_buffers() {
    const dnnca_model_desc& d = desc;
    const size_t MB = (size_t)d.max_batch;
    // flat buffers
    DN_TRY(alloc((void**)&p, (size_t)nT * 4));
    DN_TRY(alloc((void**)&g, (size_t)(nT + 8 + 4) * 4));
    DN_TRY(alloc((void**)&m, (size_t)nT * 4));
    DN_TRY(alloc((void**)&v, (size_t)nT * 4));
    DN_TRY(alloc((void**)&state, (size_t)nS * 4));
    DN_TRY(alloc((void**)&scalars, kScalars * 8));
    out5 = g + nT;
    size_t npix = MB * outH * outW;
    DN_TRY(alloc((void**)&x_stage, MB * d.height * d.width * d.in_channels * 4));
    DN_TRY(alloc((void**)&y_stage, npix * 4));
    DN_TRY(alloc((void**)&logits, npix * 4));
    DN_TRY(alloc((void**)&dlogits, npix * 4));
    DN_TRY(alloc((void**)&prob, npix * 4));
    DN_TRY(alloc((void**)&eval_thr.dev, DNNCA_CONF_MAX_THR * 4));
    DN_TRY(alloc((void**)&head_partials, 2048 * 72 * 4));
    DN_TRY(alloc((void**)&conf_dev, 2 * (DNNCA_CONF_MAX_THR + 1) * 8));     // confusion histogram / host all-reduce staging
    // Keras defaults for the non-trainable / BN variables: gamma 1, moving_variance 1 (the rest 0)
    {
        std::vector<float> hp((size_t)nT, 0.f), hs((size_t)nS, 0.f);
        for (auto& pi : params) {
            bool one = pi.name.size() > 6 && (pi.name.rfind(".gamma") == pi.name.size() - 6 ||
                                              pi.name.rfind(".moving_variance") == pi.name.size() - 16);
            if (!one) continue;
            float* dst = pi.trainable ? hp.data() : hs.data();
            for (int64_t k = 0; k < pi.size; ++k) dst[pi.offset + k] = 1.f;
        }
        if (nT) HIP_TRY(hipMemcpyAsync(p, hp.data(), (size_t)nT * 4, hipMemcpyHostToDevice, stream));
        if (nS) HIP_TRY(hipMemcpyAsync(state, hs.data(), (size_t)nS * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    return DNNCA_OK;
}


// ---------------------------------------------------------------------------------------------- MultiResUnet plan
// models/tf_models/multiresunet.py, in the order in which its code calls the layers (= Keras variable creation order):
//   conv2d_bn(x, f, k):  conv k x k, same, no bias -> BatchNorm without gamma -> ReLU | nothing        (OP_CONV, OP_BN with alpha)
//   MultiResBlock(U):    shortcut = conv2d_bn 1x1 (c1 + c2 + c3, none); a, b, c = conv2d_bn 3x3 chained (c1, c2, c3, relu);
//                        out = BN(concat[a, b, c]); out = BN(relu(shortcut + out))                      (OP_JOIN + OP_BN)
//   ResPath(f, length):  length x { s = conv2d_bn 1x1 (none); o = conv2d_bn 3x3 (relu); x = BN(relu(s + o)) }
// Concats are never materialised: a, b, c are channel slices of one tensor that the concat BatchNorm reads whole; the decoder's
// concat[tconv, respath] is the two-source input (inA, inB) of the block's shortcut conv and first 3x3 conv.
static void multires_widths(int U, int* c1, int* c2, int* c3) {
    const double W = 1.67 * U;          // evaluated in double, as Python does (alpha = 1.67)
    *c1 = (int)(W * 0.167);
    *c2 = (int)(W * 0.333);
    *c3 = (int)(W * 0.5);
}

int Model::build_multires() {
    dnnca_model_desc& d = desc;
    if (d.in_channels < 1 || d.n_filters_first < 1 || d.max_batch < 1 || d.height < 1 || d.width < 1) { set_error("bad model_options"); return DNNCA_EINVAL; }
    if (d.dtype != DNNCA_F32) { set_error("MultiResUnet runs in dtype f32 only (bf16 is not implemented for this model)"); return DNNCA_EINVAL; }
    if (d.height % 16 || d.width % 16) { set_error("MultiResUnet: H, W (%d, %d) must be multiples of 16 (four 2x2 poolings)", d.height, d.width); return DNNCA_EINVAL; }
    for (int l = 0, U = d.n_filters_first; l < 5; ++l, U *= 2) {
        int c1, c2, c3;
        multires_widths(U, &c1, &c2, &c3);
        if (c1 < 1 || c2 < 1 || c3 < 1) { set_error("MultiResUnet: n_filters_first %d gives an empty conv at U = %d (widths %d, %d, %d)", d.n_filters_first, U, c1, c2, c3); return DNNCA_EINVAL; }
    }
    // the arch implies what FLAG_GENERIC implies: no tuned launcher and no fused, riding or elided arm takes an op of this plan
    // (its widths are no multiples of 16, its convs have no bias and its BatchNorms no gamma); the joins have kernels of their own
    d.flags |= 1;
    d.n_downsample = 4; d.rate = 2; d.kernel_size = 3; d.conv_stride = 1; d.bn = 1; d.padding = DNNCA_PAD_SAME;
    d.n_conv = 3; d.leaky_alpha = 0.f; d.l2 = 0.f; d.reference_index = 0;

    int rc = DNNCA_OK;
    auto tensor = [&](int H, int W, int C) { return this->new_tensor(H, W, C, &rc); };
    xin.d.H = d.height; xin.d.W = d.width; xin.d.C = d.in_channels; xin.d.ps = d.in_channels;
    xin.g = xin.d;
    const T none;                        // C = 0
    bool reads_input = true;             // until the first block's two convs of the network input have been added

    auto bn = [&](const std::string& prefix, const T& in, const T& out, bool gamma, float alpha) {
        Op o;
        o.type = OP_BN;
        o.name = prefix;
        o.inA = in;
        o.out = out;
        o.alpha = alpha;
        const int C = in.d.C;
        if (gamma) o.w_off = add_param(prefix + ".gamma", {C}, 1);
        o.b_off = add_param(prefix + ".beta", {C}, 1);
        o.mm_off = add_param(prefix + ".moving_mean", {C}, 0);
        o.mv_off = add_param(prefix + ".moving_variance", {C}, 0);
        if (rc == DNNCA_OK) rc = alloc((void**)&o.coef, (size_t)4 * C * 4);
        if (rc == DNNCA_OK) rc = alloc((void**)&o.ws, (size_t)2 * C * 8);
        if (!gamma) nogamma_n += (size_t)C;
        ops.push_back(o);
    };
    // conv2d_bn: `out` receives the BatchNorm's (activated) output
    auto conv_bn = [&](const std::string& prefix, const T& inA, const T& inB, const T& out, int k, float alpha) {
        Op o;
        o.type = OP_CONV;
        o.name = prefix;
        o.inA = inA;
        o.inB = inB;
        o.out = tensor(out.d.H, out.d.W, out.d.C);
        o.k = k;
        o.alpha = -1.f;
        o.need_din = !reads_input;
        o.w_off = add_param(prefix + ".kernel", {k, k, inA.d.C + inB.d.C, out.d.C}, 1);
        ops.push_back(o);
        bn(prefix + ".bn", o.out, out, false, alpha);
    };
    auto join_bn = [&](const std::string& prefix, const T& a, const T& b) -> T {
        Op o;
        o.type = OP_JOIN;
        o.name = prefix + ".join";
        o.inA = a;
        o.inB = b;
        o.out = tensor(a.d.H, a.d.W, a.d.C);
        ops.push_back(o);
        T out = tensor(a.d.H, a.d.W, a.d.C);
        bn(prefix + ".out_bn", o.out, out, true, -1.f);
        return out;
    };
    auto block = [&](const std::string& p, int U, const T& inA, const T& inB) -> T {
        int c1, c2, c3;
        multires_widths(U, &c1, &c2, &c3);
        const int H = inA.d.H, W = inA.d.W, Cs = c1 + c2 + c3;
        T shortcut = tensor(H, W, Cs), cat = tensor(H, W, Cs), cat_n = tensor(H, W, Cs);
        const T a = tslice(cat, 0, c1), b = tslice(cat, c1, c2), c = tslice(cat, c1 + c2, c3);
        conv_bn(p + ".shortcut", inA, inB, shortcut, 1, -1.f);
        conv_bn(p + ".conv3", inA, inB, a, 3, 0.f);
        reads_input = false;
        conv_bn(p + ".conv5", a, none, b, 3, 0.f);
        conv_bn(p + ".conv7", b, none, c, 3, 0.f);
        bn(p + ".cat_bn", cat, cat_n, true, -1.f);
        return join_bn(p, shortcut, cat_n);
    };
    auto respath = [&](const std::string& p, int f, int length, T x) -> T {
        for (int i = 0; i < length; ++i) {
            const std::string q = p + "." + std::to_string(i);
            T s = tensor(x.d.H, x.d.W, f), o = tensor(x.d.H, x.d.W, f);
            conv_bn(q + ".shortcut", x, none, s, 1, -1.f);
            conv_bn(q + ".conv", x, none, o, 3, 0.f);
            x = join_bn(q, s, o);
        }
        return x;
    };

    const int U0 = d.n_filters_first;
    T cur = xin, skip[4];
    for (int l = 0; l < 5; ++l) {
        const std::string n = std::to_string(l + 1);
        T out = block("block" + n, U0 << l, cur, none);
        if (l == 4) { cur = out; break; }
        Op o;
        o.type = OP_POOL;
        o.name = "pool" + n;
        o.inA = out;
        o.out = tensor(out.d.H / 2, out.d.W / 2, out.d.C);
        o.k = 2;
        ops.push_back(o);
        cur = o.out;
        skip[l] = respath("respath" + n, U0 << l, 4 - l, out);
    }
    for (int u = 0; u < 4; ++u) {
        const int l = 3 - u, U = U0 << l;
        const std::string n = std::to_string(6 + u);
        Op o;
        o.type = OP_TCONV;
        o.name = "up" + n + ".tconv";
        o.inA = cur;
        o.out = tensor(cur.d.H * 2, cur.d.W * 2, U);
        o.k = 2;
        o.w_off = add_param("up" + n + ".tconv.kernel", {2, 2, U, cur.d.C}, 1);
        o.b_off = add_param("up" + n + ".tconv.bias", {U}, 1);
        ops.push_back(o);
        cur = block("block" + n, U, o.out, skip[l]);
    }
    // head: conv2d_bn 1x1 -> 1 channel; the logits the loss consumes are the output of that BatchNorm (losses.py reads
    // y_pred._keras_logits), the sigmoid is the loss kernel's / g_sigmoid's
    T head = tensor(d.height, d.width, 1);
    conv_bn("head", cur, none, head, 1, -1.f);
    outH = d.height;
    outW = d.width;
    if (rc != DNNCA_OK) return rc;

    // sum(dy xhat) of the BatchNorms without gamma, and the partial table of the widest join
    DN_TRY(alloc((void**)&nogamma_scratch, (nogamma_n + 4) * 4));
    size_t at = 0, part = 1;
    for (Op& o : ops) {
        if (o.type == OP_BN && o.w_off < 0) { o.nogamma_sum = nogamma_scratch + at; at += (size_t)o.inA.d.C; }
        if (o.type == OP_JOIN) part = std::max(part, join_part_doubles(o.out.d.C));
    }
    DN_TRY(alloc((void**)&join_part, part * 8));
    DN_TRY(alloc((void**)&join_ticket, 16));

    // backward accumulation flags: the first op (in backward order) to produce a gradient overwrites, later ones add -- by channel
    // INTERVAL of the gradient buffer, not by pointer: the concat BatchNorm's backward writes slices a, b and c through the base
    // pointer, which only slice a shares, so conv7's backward must ADD to slice b.  A later writer must lie inside what an earlier
    // one wrote (a wider one would add to channels nobody has written)
    struct Span { const float* p; int C; };
    std::vector<Span> written;
    int bad = 0;
    auto claim = [&](const View& g) -> bool {
        bool overlap = false, inside = false;
        for (const Span& w : written) {
            if (g.p < w.p + w.C && w.p < g.p + g.C) overlap = true;
            if (g.p >= w.p && g.p + g.C <= w.p + w.C) inside = true;
        }
        if (overlap && !inside) ++bad;
        if (!inside) written.push_back(Span{g.p, g.C});
        return overlap;
    };
    for (int i = (int)ops.size() - 1; i >= 0; --i) {
        Op& o = ops[i];
        if (!o.need_din) continue;
        o.accA = claim(o.inA.g);
        if ((o.type == OP_CONV || o.type == OP_JOIN) && o.inB.d.C) o.accB = claim(o.inB.g);
    }
    if (bad) { set_error("internal: MultiResUnet plan: %d gradient writers partly overlap an earlier one", bad); return DNNCA_ESTATE; }
    // what the forward pass relies on: the op behind a join is the BatchNorm (with gamma) of the joined tensor
    for (size_t i = 0; i < ops.size(); ++i) {
        if (ops[i].type != OP_JOIN) continue;
        const bool ok = i + 1 < ops.size() && ops[i + 1].type == OP_BN && ops[i + 1].inA.d.p == ops[i].out.d.p &&
                        ops[i + 1].inA.d.C == ops[i].out.d.C && ops[i + 1].w_off >= 0;
        if (!ok) { set_error("internal: MultiResUnet plan: %s is not followed by its BatchNorm", ops[i].name.c_str()); return DNNCA_ESTATE; }
    }

    DN_TRY(build_buffers());
    // the head BatchNorm's output and output gradient ARE the logits and their gradient
    logits = ops.back().out.d.p;
    dlogits = ops.back().out.g.p;
    return DNNCA_OK;
}

// ---------------------------------------------------------------------------------------------- forward
static inline double nelem(int B, const View& v) { return (double)B * v.H * v.W * v.C; }

// the untuned kernels read and write f32 only: a tensor stored as bf16 (View::h) must have been taken by a tuned kernel
static bool all_f32(const Op& o) {
    if (!(o.inA.d.h | o.inA.g.h | o.inB.d.h | o.inB.g.h | o.out.d.h | o.out.g.h)) return true;
    set_error("internal: %s has a bf16-stored operand but no tuned kernel took it", o.name.c_str());
    return false;
}

bool Model::lockstep() const {
    // OFF by default: nothing shares a launch across the encoders yet, and the order alone costs cache locality (pass_order).
    // DNNCA_LOCKSTEP=1 walks the encoders in lockstep (the groundwork for one launch per twin-op triple; results are unchanged).
    return sw.lockstep && enc_ops > 0 && !(desc.flags & 1);
}

std::vector<int> Model::pass_order(bool backward) const {
    std::vector<int> ord;
    const int n = (int)ops.size(), ne = lockstep() && !(backward && step.bucketing) ? enc_ops * n_enc : 0;
    // Only the levels whose tensors are small walk in lockstep: at full resolution an op's output (134 MB at 8 x 512 x 512 x 16) is
    // what the next op of the SAME encoder reads, largely out of the 256 MB Infinity Cache; with the other encoders' ops in between it
    // comes from HBM.  Measured on mulmo_unet (8.93 ms sequential, same box): lockstep over all four levels 9.23 ms, levels <= 256^2
    // 9.14, <= 128^2 9.00, <= 64^2 9.02 -- so only the two deep levels are candidates for shared launches.
    const int max_h = sw.lockstep_maxh;
    int j0 = 0;          // first op (relative index) of the lockstep part
    while (ne && j0 < enc_ops && ops[j0].out.d.H > max_h) ++j0;
    if (!backward) {
        for (int e = 0; e < (ne ? n_enc : 0); ++e)
            for (int j = 0; j < j0; ++j) ord.push_back(e * enc_ops + j);
        for (int j = j0; j < (ne ? enc_ops : 0); ++j)
            for (int e = 0; e < n_enc; ++e) ord.push_back(e * enc_ops + j);
        for (int i = ne; i < n; ++i) ord.push_back(i);
    } else {
        for (int i = n - 1; i >= ne; --i) ord.push_back(i);
        for (int j = (ne ? enc_ops : 0) - 1; j >= j0; --j)
            for (int e = n_enc - 1; e >= 0; --e) ord.push_back(e * enc_ops + j);
        for (int e = (ne ? n_enc : 0) - 1; e >= 0; --e)
            for (int j = j0 - 1; j >= 0; --j) ord.push_back(e * enc_ops + j);
    }
    return ord;
}

int Model::forward(const float* x_dev, int B, bool training, const StepRequest& req) {
    if (B < 1 || B > desc.max_batch) { set_error("batch %d outside [1, max_batch=%d]", B, desc.max_batch); return DNNCA_EINVAL; }
    last_batch = B;
    if (!dry && !sens_pass) tta_spread_valid = false;   // the probabilities are about to change (dnnca_forward_tta_spread sets it again)
    // (the input-sensitivity pass walks the per-op arms too: every tensor its backward pass reads is then stored)
    const bool generic = (desc.flags & 1) || sens_pass;
    // input ops carry a channel offset relative to xin; rebase them on this batch
    for (Op& o : ops)
        if (o.type == OP_CONV && !o.need_din) {
            ptrdiff_t off = o.inA.d.p - xin.d.p;
            o.inA.d.p = const_cast<float*>(x_dev) + off;
        }
    xin.d.p = const_cast<float*>(x_dev);
    step = Step{};          // a pass begins: no hand-over of an earlier step, finished or stopped on an error, survives this line
    if (!sens_pass) DN_TRY(fast_prepare(this, req.defer_head));
    DN_TRY(ig_prepare(this));
    // the head will ride in the last conv's epilogue: it needs the label statistics (positive rate) of this step, so they go first
    // (pg_prep has just zeroed the scalars)
    bool head_in_conv_ok = req.head_in_conv && !generic && (step.step_init_done || dry) && head_defer_ok && ops.size() >= 2 &&
                           ops.back().type == OP_HEAD && fast_head_supported(this, ops.back());
    // ... either from the first encoder block's fused launch (when the head-in-conv kernel will be there to consume its partials
    // table; the label image is then the network's output geometry: the first block runs at full resolution) or from their own kernel
    const float* labels_in_first_block = nullptr;
    if (head_in_conv_ok) {
        if (!sw.no_label_fusion && fast_head_in_conv_possible(this) && ops[0].type == OP_CONV && !ops[0].need_din && ops[0].out.d.H == outH &&
            ops[0].out.d.W == outW)
            labels_in_first_block = req.y;
        else
            head_in_conv_ok = fast_label_stats(this, (size_t)B * outH * outW, req.y);
    }
    step.head_in_conv.y = req.y;
    step.head_in_conv.labels_done = head_in_conv_ok;

    // op_done[i]: op i's work rode in an earlier launch of this pass (a max-pool in the preceding conv's / BatchNorm's launch, the
    // later layers of a fused block, the twin ops of the other mulmo encoders)
    const std::vector<int> order = pass_order(false);
    step.op_done.assign(ops.size(), 0);
    for (size_t ok_ = 0; ok_ < order.size(); ++ok_) {
        size_t oi = (size_t)order[ok_];
        if (step.op_done[oi]) continue;
        Op& o = ops[oi];
        cur_op = &o.name;
        switch (o.type) {
            case OP_CONV: {
                int Cin = o.inA.d.C + o.inB.d.C;
                double bytes = 4.0 * (nelem(B, o.inA.d) + nelem(B, o.inB.d) + nelem(B, o.out.d));
                double flops = 2.0 * B * o.out.d.H * o.out.d.W * o.k * o.k * Cin * o.out.d.C;
                if (head_in_conv_ok && oi + 2 == ops.size()) {                // the conv that feeds the head: head + loss + head backward in its epilogue
                    const float gs = (float)(1.0 / ((double)outH * outW * B));
                    const double npx = (double)B * outH * outW;
                    if (fast_tail3(this, B, o, ops.back(), req.y, req.cfg, gs) ||
                        fast_conv_fwd_head(this, B, o, ops.back(), req.y, req.cfg, gs, bytes + 4.0 * npx * (1 + o.out.d.C), flops + 30.0 * npx)) {
                        step.head_in_conv.done = true;
                        break;
                    }
                    if (step.label_part_valid) { set_error("internal: label partials without the head-in-conv kernel"); return DNNCA_ESTATE; }
                }
                if (oi == 0 && labels_in_first_block) {
                    if (!generic && fused_down_fwd(this, B, oi, training, labels_in_first_block)) {
                        step.op_done[oi + 1] = step.op_done[oi + 2] = 1;
                        break;
                    }
                    // the first block did not take them: the label statistics get their own launch after all
                    head_in_conv_ok = fast_label_stats(this, (size_t)B * outH * outW, req.y);
                    step.head_in_conv.labels_done = head_in_conv_ok;
                    labels_in_first_block = nullptr;
                }
                if (!generic && fused_down_fwd(this, B, oi, training)) {      // conv, conv, pool of one encoder block in one launch
                    step.op_done[oi + 1] = step.op_done[oi + 2] = 1;
                    break;
                }
                if (!generic && o.inB.d.C && fused_up2_fwd(this, B, oi, training)) {      // the two convs of a decoder block (its transposed conv rode earlier)
                    step.op_done[oi + 1] = 1;
                    break;
                }
                Op* pool = (!generic && oi + 1 < ops.size() && fast_pool_fusable(this, o, ops[oi + 1])) ? &ops[oi + 1] : nullptr;
                if (!generic && fast_conv_fwd(this, B, o, bytes + (pool ? 4.0 * nelem(B, pool->out.d) : 0.0), flops, pool)) {
                    if (pool) step.op_done[pool - ops.data()] = 1;
                    break;
                }
                Op* bn_next = (training && oi + 1 < ops.size() && ops[oi + 1].type == OP_BN && ops[oi + 1].inA.d.p == o.out.d.p &&
                               fast_bn_supported(this, ops[oi + 1])) ? &ops[oi + 1] : nullptr;
                if (!generic && (fast_first_conv_fwd(this, B, o, bytes, flops, bn_next) || ig_conv_fwd(this, B, o, bytes, flops, bn_next))) break;
                if (sens_pass && !(desc.flags & 1) && ig_conv_fwd(this, B, o, bytes, flops, nullptr)) break;      // dense conv, output stored, nothing riding
                if (!all_f32(o)) return DNNCA_ESTATE;
                LAUNCH(this, "g_conv_fwd", bytes, flops,
                       g_conv_fwd(stream, B, o.inA.d, o.inB.d, p + o.w_off, o.b_off >= 0 ? p + o.b_off : nullptr, o.out.d, o.k, o.alpha));
                break;
            }
            case OP_BN: {
                int C = o.inA.d.C;
                double n = (double)B * o.inA.d.H * o.inA.d.W;
                double tb = 4.0 * nelem(B, o.inA.d);
                Op* bn_pool = (!generic && oi + 1 < ops.size() && fast_bn_pool_fusable(this, o, ops[oi + 1])) ? &ops[oi + 1] : nullptr;
                // every reader a conv that normalises while it stages its operands: no apply pass, no normalised tensor
                o.elided = false;
                if (!generic && !bn_pool && !o.out_readers.empty() && fast_bn_supported(this, o)) {
                    bool all = true;
                    for (int r : o.out_readers) all = all && r >= 0 && ops[r].type == OP_CONV && ig_norm_on_load_ok(this, B, ops[r]);
                    o.elided = all;
                }
                Op* pool_bn = (bn_pool && training && oi + 2 < ops.size() && ops[oi + 2].type == OP_BN &&
                               ops[oi + 2].inA.d.p == bn_pool->out.d.p && fast_bn_supported(this, ops[oi + 2])) ? &ops[oi + 2] : nullptr;
                if (!generic && fast_bn_fwd(this, B, o, training, kBnMomentum, kBnEps, bn_pool, pool_bn)) {
                    if (bn_pool) step.op_done[bn_pool - ops.data()] = 1;
                    break;
                }
                if (!all_f32(o)) return DNNCA_ESTATE;
                if (training) {
                    if (!o.mean_ready) {          // (else: join_fwd left the sums and zeroed the squares' row)
                        if (!dry) HIP_TRY(hipMemsetAsync(o.ws, 0, (size_t)2 * C * 8, stream));
                        LAUNCH(this, "g_bn_stats_mean", tb, tb / 4, g_bn_stats_mean(stream, B, o.inA.d, o.ws));
                    }
                    o.mean_ready = false;
                    LAUNCH(this, "g_bn_stats_var", tb, tb / 2, g_bn_stats_var(stream, B, o.inA.d, o.ws));
                }
                LAUNCH(this, "g_bn_finalize", 0, 0,
                       g_bn_finalize(stream, C, n, o.ws, o.w_off >= 0 ? p + o.w_off : nullptr, p + o.b_off, state + o.mm_off, state + o.mv_off,
                                     o.coef, training ? 1 : 0, kBnMomentum, kBnEps));
                LAUNCH(this, "g_bn_apply", 2 * tb, tb / 2, g_bn_apply(stream, B, o.inA.d, o.out.d, o.coef, o.alpha));
                break;
            }
            case OP_JOIN: {
                // out = relu(inA + inB); the BatchNorm behind it is ops[oi + 1] (build_multires)
                const double tb = 4.0 * nelem(B, o.out.d);
                Op& nb = ops[oi + 1];
                if (sw.no_join) {
                    LAUNCH(this, "g_join_fwd", 3 * tb, tb / 4, g_join_fwd(stream, B, o.inA.d, o.inB.d, o.out.d));
                    break;
                }
                if (training) {
                    // one pass: the joined tensor and the channel sums of the BatchNorm's mean; the BatchNorm's own arm runs the
                    // variance pass, finalize and apply
                    LAUNCH(this, "join_fwd", 3 * tb, tb / 2, join_fwd(stream, B, o.inA.d, o.inB.d, o.out.d, nb.ws, join_part, join_ticket));
                    nb.mean_ready = true;
                    break;
                }
                // inference: add, ReLU and the BatchNorm's affine from the moving statistics in one pass; the joined tensor is not stored
                LAUNCH(this, "g_bn_finalize", 0, 0,
                       g_bn_finalize(stream, nb.inA.d.C, 1.0, nb.ws, p + nb.w_off, p + nb.b_off, state + nb.mm_off, state + nb.mv_off,
                                     nb.coef, 0, kBnMomentum, kBnEps));
                LAUNCH(this, "join_infer", 3 * tb, tb, join_infer(stream, B, o.inA.d, o.inB.d, nb.out.d, nb.coef));
                step.op_done[oi + 1] = 1;
                break;
            }
            case OP_POOL: {
                // (a pool computed by the launch that produced its input never gets here: op_done)
                double bytes = 4.0 * (nelem(B, o.inA.d) + nelem(B, o.out.d));
                if (!generic && fast_pool_fwd(this, B, o, bytes)) break;
                if (!all_f32(o)) return DNNCA_ESTATE;
                LAUNCH(this, "g_pool_fwd", bytes, 0, g_pool_fwd(stream, B, o.inA.d, o.out.d, o.k));
                break;
            }
            case OP_TCONV: {
                double bytes = 4.0 * (nelem(B, o.inA.d) + nelem(B, o.out.d));
                double flops = 2.0 * nelem(B, o.out.d) * o.inA.d.C;
                int used = 3;
                if (!generic && fused_up_fwd(this, B, oi, training, &used)) { // tconv, conv, conv of one decoder block in one launch
                    for (int t = 1; t < used; ++t) step.op_done[oi + t] = 1;       // (+ the next block's tconv when it rides along)
                    break;
                }
                if (!generic && fast_up3_fwd(this, B, oi)) {                  // tconv + two-source conv of the 3-channel level
                    step.op_done[oi + 1] = 1;
                    break;
                }
                Op* bn_next = (training && oi + 1 < ops.size() && ops[oi + 1].type == OP_BN && ops[oi + 1].inA.d.p == o.out.d.p &&
                               fast_bn_supported(this, ops[oi + 1])) ? &ops[oi + 1] : nullptr;
                if (!generic && (fast_tconv_fwd(this, B, o, bytes, flops) || ig_tconv_fwd(this, B, o, bytes, flops, bn_next))) break;
                if (sens_pass && !(desc.flags & 1) && ig_tconv_fwd(this, B, o, bytes, flops, nullptr)) break;
                if (!all_f32(o)) return DNNCA_ESTATE;
                LAUNCH(this, "g_tconv_fwd", bytes, flops,
                       g_tconv_fwd(stream, B, o.inA.d, p + o.w_off, p + o.b_off, o.out.d, o.k));
                break;
            }
            case OP_HEAD: {
                double npix = (double)B * outH * outW;
                if (req.defer_head && !generic && fast_head_supported(this, o)) {
                    step.head_deferred = true;   // runs fused with the loss and its own backward (fast_head_train)
                    break;
                }
                if (!all_f32(o)) return DNNCA_ESTATE;
                LAUNCH(this, "g_head_fwd", 4.0 * (nelem(B, o.inA.d) + npix), 2.0 * nelem(B, o.inA.d),
                       g_head_fwd(stream, B, o.inA.d, p + o.w_off, p + o.b_off, sens_pass ? dlogits : logits));
                break;
            }
        }
    }
    return DNNCA_OK;
}

// ---------------------------------------------------------------------------------------------- loss + backward
int Model::loss_and_backward(const float* y_dev, int B, const dnnca_loss_cfg& cfg, bool backward) {
    cur_op = nullptr;
    // the partial sums of a head that ran in this step's forward pass wait for the fold; no other head's do (that head runs again)
    if (!(backward && step.head_in_conv.done && y_dev == step.head_in_conv.y)) step.head_pending.partials = nullptr;
    const float* y_raw = y_dev;         // the boundary term's distance map comes from the labels before the blur
    if (cfg.label_smoothing) {          // utils/losses.py:62-67: every later use of y_true (positive rate, assertions, loss) sees the blurred labels
        if (!y_smooth) DN_TRY(alloc((void**)&y_smooth, (size_t)desc.max_batch * outH * outW * 4));
        if (!fast_label_smooth(this, B, outH, outW, y_dev, y_smooth, cfg.label_smoothing_filter_size, cfg.label_smoothing_sigma)) {
            set_error("label_smoothing: filter size %d / sigma %g not supported for %dx%d labels", cfg.label_smoothing_filter_size,
                      (double)cfg.label_smoothing_sigma, outH, outW);
            return DNNCA_EINVAL;
        }
        y_dev = y_smooth;
    }
    const bool generic = desc.flags & 1;
    size_t npix = (size_t)B * outH * outW;
    const bool labels_done = backward && step.head_in_conv.labels_done && y_dev == step.head_in_conv.y;
    const bool head_was_in_conv = labels_done && step.head_in_conv.done;
    step.head_in_conv.labels_done = step.head_in_conv.done = false;          // consumed: this pass is the one they were run for
    // scalars: label sum 0, min +inf, max -inf, loss 0, l2 0
    if (!(step.step_init_done && backward))
        LAUNCH(this, "g_step_init", 0, 0,
               g_step_init(stream, scalars, g, backward ? (size_t)(nT + 8) : 0, multires() ? nogamma_scratch : extra_zero,
                           !backward ? 0 : (multires() ? nogamma_n : (generic ? 0 : extra_zero_n))));
    step.step_init_done = false;          // consumed, whether or not g_step_init ran
    if (labels_done) {
        // the forward pass of this train step already ran the label statistics (and maybe the head, in its last conv's epilogue)
    } else if (generic || !fast_label_stats(this, npix, y_dev))
        LAUNCH(this, "g_label_stats", 4.0 * npix, (double)npix, g_label_stats(stream, npix, y_dev, scalars));
    // dlogits scale: mean over (H, W), then mean over the (rank-local) batch.  Under data parallel every rank uses its
    // local mean; the cross-rank 1/world is applied to the all-reduced gradient in the optimizer step.
    float gscale = (float)(1.0 / ((double)outH * outW * B));
    bool head_done = false;
    if (region_loss.on) {
        // the region (Tversky) term: sums per image first, then the gradient (kernels_region_loss.hip)
        if (head_was_in_conv) { set_error("internal: region loss behind a head that ran in the forward pass"); return DNNCA_ESTATE; }
        if (boundary.weight > 0.f) {     // the signed distance map of this step's raw labels, a constant of the step (kernels_boundary.hip)
            boundary_transform(this, y_raw, B, outH, outW, boundary.cols, boundary.phi, nullptr);
            if (!dry) boundary.batch = B;
        }
        if (backward && step.head_deferred) {
            if (!region_loss_head_train(this, B, ops.back(), y_dev, cfg, gscale)) {
                set_error("internal: deferred head has no region-loss kernel");
                return DNNCA_ESTATE;
            }
            head_done = true;
        } else {
            DN_TRY(region_loss_from_logits(this, B, y_dev, cfg, gscale, backward ? dlogits : nullptr));
        }
    } else if (head_was_in_conv) {
        head_done = true;
    } else if (backward && step.head_deferred) {
        Op& ho = ops.back();
        double fb = 4.0 * nelem(B, ho.inA.d);
        if (!fast_head_train(this, B, ho, y_dev, cfg, gscale, 2 * fb + 4.0 * npix)) {
            set_error("internal: deferred head has no fused kernel");
            return DNNCA_ESTATE;
        }
        head_done = true;
    } else {
        LAUNCH(this, "g_loss", 4.0 * npix * (backward ? 4 : 3), 20.0 * npix,
               g_loss(stream, npix, logits, y_dev, cfg, (double)npix, scalars, backward ? dlogits : nullptr, prob, gscale));
    }
    if (backward) {
        cur_op = nullptr;
        DN_TRY(ig_begin_backward(this));
        // bucketed gradient all-reduce (data parallel, large models): see model.h.  Not for the pixel-group plan (its slabs are
        // folded into the gradient vector by the launch that ENDS the backward pass; 34.7 KB anyway) and not with an L2
        // regulariser (its gradient is added after the loop).
        collectives_last_step = 0;
        // Nor with gradient accumulation: buckets would reduce this micro-step's g, not the accumulator.
        if (comm && !dry && (size_t)nT * 4 > (1u << 20) && desc.l2 == 0.f && !head_defer_ok && !accum.a) {
            if (bucket_state == 0) {
                int64_t prev = -1;
                bucket_state = 1;
                for (const Op& q : ops) {
                    int64_t lo = q.w_off >= 0 ? q.w_off : q.b_off;
                    if (q.b_off >= 0 && q.b_off < lo) lo = q.b_off;
                    if (lo < 0) continue;
                    if (lo <= prev) { bucket_state = -1; break; }
                    prev = lo;
                }
            }
            step.bucketing = bucket_state == 1;
            step.bucket_hi = step.bucket_fin = nT;
        }
        const std::vector<int> order = pass_order(true);          // (lockstep over the mulmo encoders unless this pass sends gradient buckets)
        step.op_done.assign(ops.size(), 0);
        for (size_t ok_ = 0; ok_ < order.size(); ++ok_) {
            const int i = order[ok_];
            if (step.op_done[i]) continue;
            Op& o = ops[i];
            cur_op = &o.name;
            if (step.bucketing && i + 1 < (int)ops.size()) {
                // everything from the previous (later) op's parameters to the end of the vector is final now
                const Op& d = ops[i + 1];
                int64_t lo = d.w_off >= 0 ? d.w_off : d.b_off;
                if (d.b_off >= 0 && d.b_off < lo) lo = d.b_off;
                if (lo >= 0 && lo < step.bucket_fin) step.bucket_fin = lo;
                if ((size_t)(step.bucket_hi - step.bucket_fin) * 4 >= sw.bucket_bytes) {
                    DN_TRY(send_bucket(step.bucket_fin, step.bucket_hi));
                    step.bucket_hi = step.bucket_fin;
                }
            }
            switch (o.type) {
                case OP_HEAD: {
                    if (head_done) break;
                    if (o.maskA) { set_error("internal: masked head gradient needs the fused kernel"); return DNNCA_ESTATE; }
                    double fb = 4.0 * nelem(B, o.inA.d);
                    LAUNCH(this, "g_head_bwd", 2 * fb + 4.0 * npix, 4.0 * nelem(B, o.inA.d),
                           g_head_bwd(stream, B, o.inA.d, p + o.w_off, dlogits, o.inA.g, g + o.w_off, g + o.b_off));
                    break;
                }
                case OP_CONV: {
                    int Cin = o.inA.d.C + o.inB.d.C;
                    double ob = 4.0 * nelem(B, o.out.d), ib = 4.0 * (nelem(B, o.inA.d) + nelem(B, o.inB.d));
                    double flops = 2.0 * B * o.out.d.H * o.out.d.W * o.k * o.k * Cin * o.out.d.C;
                    if (step.first_done == &o) {                         // its weight gradient rode in the previous launch (k_first3)
                        step.first_done = nullptr;
                        break;
                    }
                    if (step.tail_done == &o && head_was_in_conv) {      // its backward ran with the head, inside the forward pass (fast_tail3)
                        step.tail_done = nullptr;
                        break;
                    }
                    if (!generic && i >= 2 && fused_up_bwd(this, B, (size_t)i)) {       // second conv, first conv, transposed conv of a decoder block in one launch
                        step.op_done[i - 1] = step.op_done[i - 2] = 1;
                        break;
                    }
                    if (!generic && (fast_conv_bwd(this, B, o, ob, ib, flops) || fast_first_conv_bwd(this, B, o, ob, ib, flops) ||
                                     ig_conv_bwd(this, B, o, ob, ib, flops))) break;
                    if (!all_f32(o)) return DNNCA_ESTATE;
                    if (o.maskA || o.maskB) { set_error("internal: masked conv gradient has no tuned kernel"); return DNNCA_ESTATE; }
                    if (o.alpha >= 0.f && !o.premasked)
                        LAUNCH(this, "g_act_bwd", 3 * ob, ob / 4,
                               g_act_bwd(stream, (size_t)nelem(B, o.out.d), o.out.g.p, o.out.d.p, o.alpha));
                    LAUNCH(this, "g_conv_wgrad", ob + ib, flops,
                           g_conv_wgrad(stream, B, o.inA.d, o.inB.d, o.out.g, g + o.w_off, o.b_off >= 0 ? g + o.b_off : nullptr, o.k));
                    if (o.need_din)
                        LAUNCH(this, "g_conv_dgrad", ob + ib, flops,
                               g_conv_dgrad(stream, B, o.out.g, p + o.w_off, o.inA.g, o.accA, o.inB.g, o.accB, o.k));
                    break;
                }
                case OP_BN: {
                    double tb = 4.0 * nelem(B, o.inA.d);
                    double n = (double)B * o.inA.d.H * o.inA.d.W;
                    if (!generic && fast_bn_bwd(this, B, o)) break;
                    if (!all_f32(o)) return DNNCA_ESTATE;
                    if (o.maskA) { set_error("internal: masked batch-norm gradient has no tuned kernel"); return DNNCA_ESTATE; }
                    // (MultiResUnet) conv -> BatchNorm -> ReLU: the activation's derivative first, in place on the output gradient
                    if (o.alpha >= 0.f)
                        LAUNCH(this, "g_act_bwd", 3 * tb, tb / 4, g_act_bwd_view(stream, B, o.out.g, o.out.d, o.alpha));
                    // a BatchNorm without gamma still needs sum(dy xhat) for its data gradient: it goes to the op's scratch row
                    float* dgamma = o.w_off >= 0 ? g + o.w_off : o.nogamma_sum;
                    LAUNCH(this, "g_bn_bwd_reduce", 2 * tb, tb,
                           g_bn_bwd_reduce(stream, B, o.inA.d, o.out.g, o.coef, dgamma, g + o.b_off));
                    LAUNCH(this, "g_bn_bwd_apply", 3 * tb, 2 * tb,
                           g_bn_bwd_apply(stream, B, o.inA.d, o.out.g, o.inA.g, o.accA, o.coef, o.w_off >= 0 ? p + o.w_off : nullptr, dgamma,
                                          g + o.b_off, n));
                    break;
                }
                case OP_JOIN: {
                    const double tb = 4.0 * nelem(B, o.out.d);
                    if (sw.no_join)
                        LAUNCH(this, "g_join_bwd", (4 + o.accA + o.accB) * tb, tb / 4,
                               g_join_bwd(stream, B, o.out.g, o.out.d, o.inA.g, o.accA, o.inB.g, o.accB));
                    else
                        LAUNCH(this, "join_bwd", (4 + o.accA + o.accB) * tb, tb / 4,
                               join_bwd(stream, B, o.out.g, o.out.d, o.inA.g, o.accA, o.inB.g, o.accB));
                    break;
                }
                case OP_POOL: {
                    double bytes = 4.0 * (2 * nelem(B, o.inA.d) + 2 * nelem(B, o.out.d));
                    if (!generic && i >= 2 && fused_down_bwd(this, B, (size_t)i)) {     // pool, second conv, first conv of an encoder block in one launch
                        step.op_done[i - 1] = step.op_done[i - 2] = 1;
                        break;
                    }
                    if (!generic && i > 0 && fast_pool_into_bn(this, o, ops[i - 1])) break;   // rides in the backward passes of the BatchNorm in front of it
                    if (!generic && i > 0 && fast_pool_fold(this, o, ops[i - 1])) break;      // rides in the next launch (the conv's backward)
                    if (!generic && fast_pool_bwd(this, B, o, bytes)) break;
                    if (!all_f32(o)) return DNNCA_ESTATE;
                    if (o.maskA) { set_error("internal: masked pool gradient has no tuned kernel"); return DNNCA_ESTATE; }
                    LAUNCH(this, "g_pool_bwd", bytes, 0,
                           g_pool_bwd(stream, B, o.inA.d, o.out.d, o.out.g, o.inA.g, o.accA, o.k));
                    break;
                }
                case OP_TCONV: {
                    double ob = 4.0 * nelem(B, o.out.d), ib = 4.0 * nelem(B, o.inA.d);
                    double flops = 2.0 * nelem(B, o.out.d) * o.inA.d.C;
                    if (step.tconv_done == &o) {                         // its backward rode in the previous launch (k_pgbwd TCF)
                        step.tconv_done = nullptr;
                        break;
                    }
                    if (!generic && (fast_tconv_bwd(this, B, o, ob, ib, flops) || ig_tconv_bwd(this, B, o, ob, ib, flops))) break;
                    if (!all_f32(o)) return DNNCA_ESTATE;
                    if (o.maskA) { set_error("internal: masked transposed-conv gradient has no tuned kernel"); return DNNCA_ESTATE; }
                    LAUNCH(this, "g_tconv_wgrad", ob + ib, flops,
                           g_tconv_wgrad(stream, B, o.inA.d, o.out.g, g + o.w_off, g + o.b_off, o.k));
                    LAUNCH(this, "g_tconv_dgrad", ob + ib, flops,
                           g_tconv_dgrad(stream, B, o.out.g, p + o.w_off, o.inA.g, o.accA, o.k));
                    break;
                }
            }
        }
        DN_TRY(ig_finish_wgrad(this));
        DN_TRY(wg_side_join());
        DN_TRY(fast_finish_backward(this));
        if (desc.l2 > 0.f) {
            for (auto& pi : params) {
                if (!pi.trainable || pi.name.size() < 7 || pi.name.rfind(".kernel") != pi.name.size() - 7) continue;
                LAUNCH(this, "g_l2", 12.0 * pi.size, 4.0 * pi.size,
                       g_l2(stream, (size_t)pi.size, p + pi.offset, g + pi.offset, desc.l2, scalars));
            }
        }
    } else if (desc.l2 > 0.f) {
        // evaluation: Keras adds the regulariser to the reported loss as well; it needs no gradient here.
        // (g is scratch in this mode.)
        for (auto& pi : params) {
            if (!pi.trainable || pi.name.size() < 7 || pi.name.rfind(".kernel") != pi.name.size() - 7) continue;
            LAUNCH(this, "g_l2", 12.0 * pi.size, 4.0 * pi.size,
                   g_l2(stream, (size_t)pi.size, p + pi.offset, g + pi.offset, desc.l2, scalars));
        }
    }
    if (backward && !comm && merged_launches() && (!dry || step.fold_deferred)) {
        // optimizer_step() follows every backward pass: its Adam launch also writes the step outputs (one launch fewer).  (In a dry
        // run only the deferred fold of an accumulating micro-step takes them: the plan lists that launch.)
        step.fin_pending.on = true;
        step.fin_pending.cfg = cfg;
        step.fin_pending.n_label = (double)npix;
        step.fin_pending.inv_batch_hw = 1.0 / ((double)outH * outW * B);
        return DNNCA_OK;
    }
    LAUNCH(this, "g_finalize_scalars", 0, 0,
           g_finalize_scalars(stream, scalars, cfg, (double)npix, 1.0 / ((double)outH * outW * B), out5));
    return DNNCA_OK;
}

// ---------------------------------------------------------------------------------------------- input sensitivity
// s[b, c] = sum over the image of |d sum(sigmoid(logits)) / d x[b, :, :, c]| with the model in inference mode (utils/callbacks.py:290-313):
// an inference forward that stores every tensor, then the data gradients alone over `ops` in reverse -- no weight gradient, no
// optimizer step, no BatchNorm state.  Scratch: the tensors' .g views, `dlogits` (the pass's logits: `logits` / `prob` keep the last
// forward's) and the BatchNorm coefficient tables.  The convs that read the network input get no dx tensor: one launch forms |dx| and
// reduces it (k_sens_first).

// the refusals the input-gradient passes share; `what`: the pass's name in the message
int Model::sens_refusal(const char* what) {
    if (multires()) { set_error("%s is not implemented for MultiResUnet (its pass knows the U-Net op types only)", what); return DNNCA_EINVAL; }
    if (desc.dtype != DNNCA_F32) { set_error("%s needs a dtype f32 model (this one is bf16)", what); return DNNCA_EINVAL; }
    if (desc.kernel_size > kSensMaxK) { set_error("%s: kernel_size %d above %d", what, desc.kernel_size, kSensMaxK); return DNNCA_EINVAL; }
    return DNNCA_OK;
}

// What input_sensitivity and integrated_gradients share: the inference forward of x_dev that stores every tensor (logits in
// `dlogits`), the first-layer table (built once), and the data gradients over `ops` in reverse down to the gradients of the first
// convs' outputs.  The caller launches the first-layer kernel of its choice behind it.
int Model::sens_backward(const float* x_dev, int B) {
    sens_pass = true;
    const int frc = forward(x_dev, B, false);
    sens_pass = false;
    DN_TRY(frc);
    cur_op = nullptr;
    const bool dense_ok = !(desc.flags & 1);
    const int C = desc.in_channels, H = desc.height, W = desc.width;
    if (!sens_descs) {
        std::vector<SensFirst> hd;
        for (const Op& o : ops) {
            if (o.type != OP_CONV || o.need_din) continue;
            if (o.out.d.ps != o.out.d.C || o.out.g.ps != o.out.d.C || o.inB.d.C || o.out.d.H != H || o.out.d.W != W) {
                set_error("internal: input sensitivity: %s is not a plain conv of the network input", o.name.c_str());
                return DNNCA_ESTATE;
            }
            const int chan = (int)(o.inA.d.p - xin.d.p);
            for (int c0 = 0; c0 < o.inA.d.C; c0 += kSensCi)
                hd.push_back(SensFirst{o.out.g.p, o.out.d.p, p + o.w_off, o.inA.d.C, c0, std::min(kSensCi, o.inA.d.C - c0), o.out.d.C, chan + c0, o.alpha});
        }
        if (hd.empty()) { set_error("internal: input sensitivity: no conv reads the network input"); return DNNCA_ESTATE; }
        // every network input channel belongs to exactly one entry: k_attr_first then has one writer per (pixel, channel)
        std::vector<int> owners(C, 0);
        for (const SensFirst& e : hd)
            for (int j = 0; j < e.nci; ++j) {
                if (e.chan + j < 0 || e.chan + j >= C) { set_error("internal: input sensitivity: first-layer entry outside the %d input channels", C); return DNNCA_ESTATE; }
                ++owners[e.chan + j];
            }
        for (int c = 0; c < C; ++c)
            if (owners[c] != 1) { set_error("internal: input sensitivity: input channel %d is read by %d first convs, not 1", c, owners[c]); return DNNCA_ESTATE; }
        const SensFirstGrid g = sens_first_grid(1, H, W, 1);
        void* dd = nullptr;
        DN_TRY(alloc(&dd, hd.size() * sizeof(SensFirst)));
        DN_TRY(alloc((void**)&sens_part, (size_t)desc.max_batch * C * g.ntiles * 8));
        DN_TRY(alloc((void**)&sens_ticket, (size_t)desc.max_batch * hd.size() * 4));
        DN_TRY(alloc((void**)&sens_sums, (size_t)desc.max_batch * C * 8));
        HIP_TRY(hipMemcpyAsync(dd, hd.data(), hd.size() * sizeof(SensFirst), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));          // `hd` is a local
        sens_descs = dd;
        sens_nz = (int)hd.size();
    }
    DN_TRY(ig_begin_backward(this));          // the dense data-gradient kernels read flipped weights
    for (int i = (int)ops.size() - 1; i >= 0; --i) {
        Op& o = ops[i];
        cur_op = &o.name;
        switch (o.type) {
            case OP_JOIN: break;          // (never reached: refused above)
            case OP_HEAD: {
                const double npix = (double)B * outH * outW;
                LAUNCH(this, "sens_head", 4.0 * (npix + nelem(B, o.inA.d)), 12.0 * nelem(B, o.inA.d),
                       g_sens_head(stream, B, outH, outW, dlogits, p + o.w_off, o.inA.g, o.accA));
                break;
            }
            case OP_CONV: {
                if (!o.need_din) break;          // the first layer: one launch behind the loop
                const int Cin = o.inA.d.C + o.inB.d.C;
                const double ob = 4.0 * nelem(B, o.out.d), ib = 4.0 * (nelem(B, o.inA.d) + nelem(B, o.inB.d));
                const double flops = 2.0 * B * o.out.d.H * o.out.d.W * o.k * o.k * Cin * o.out.d.C;
                if (o.out.g.h || o.out.d.h) { set_error("internal: input sensitivity met a bf16-stored tensor at %s", o.name.c_str()); return DNNCA_ESTATE; }
                if (o.alpha >= 0.f)
                    LAUNCH(this, "g_act_bwd", 3 * ob, ob / 4, g_act_bwd(stream, (size_t)nelem(B, o.out.d), o.out.g.p, o.out.d.p, o.alpha));
                if (dense_ok && ig_conv_dgrad_only(this, B, o, ob + ib, flops)) break;
                LAUNCH(this, "g_conv_dgrad", ob + ib, flops,
                       g_conv_dgrad(stream, B, o.out.g, p + o.w_off, o.inA.g, o.accA, o.inB.g, o.accB, o.k));
                break;
            }
            case OP_BN: {
                const double tb = 4.0 * nelem(B, o.inA.d);
                LAUNCH(this, "bn_infer_bwd", (o.accA ? 3 : 2) * tb, tb / 4,
                       g_bn_infer_bwd(stream, B, o.out.g, o.inA.g, o.accA, p + o.w_off, state + o.mv_off, kBnEps));
                break;
            }
            case OP_POOL: {
                const double bytes = 4.0 * (2 * nelem(B, o.inA.d) + 2 * nelem(B, o.out.d));
                LAUNCH(this, "g_pool_bwd", bytes, 0, g_pool_bwd(stream, B, o.inA.d, o.out.d, o.out.g, o.inA.g, o.accA, o.k));
                break;
            }
            case OP_TCONV: {
                const double ob = 4.0 * nelem(B, o.out.d), ib = 4.0 * nelem(B, o.inA.d);
                const double flops = 2.0 * nelem(B, o.out.d) * o.inA.d.C;
                if (dense_ok && ig_tconv_dgrad_only(this, B, o, ob + ib, flops)) break;
                LAUNCH(this, "g_tconv_dgrad", ob + ib, flops, g_tconv_dgrad(stream, B, o.out.g, p + o.w_off, o.inA.g, o.accA, o.k));
                break;
            }
        }
    }
    cur_op = nullptr;
    return DNNCA_OK;
}

// algorithmic bytes (dy and y of the first convs) and flops of one first-layer launch
void Model::sens_first_cost(int B, double* bytes, double* flops) const {
    double fb = 0, ff = 0;
    for (const Op& o : ops)
        if (o.type == OP_CONV && !o.need_din) {
            fb += 8.0 * nelem(B, o.out.d);
            ff += 2.0 * B * desc.height * desc.width * o.k * o.k * o.inA.d.C * o.out.d.C;
        }
    *bytes = fb;
    *flops = ff;
}

int Model::input_sensitivity(const float* x_dev, int B) {
    DN_TRY(sens_refusal("input sensitivity"));
    DN_TRY(sens_backward(x_dev, B));
    const int C = desc.in_channels, H = desc.height, W = desc.width;
    const SensFirstGrid g = sens_first_grid(B, H, W, sens_nz);
    double fb = 0, ff = 0;
    sens_first_cost(B, &fb, &ff);
    LAUNCH(this, "sens_first", fb, ff,
           g_sens_first(stream, (const SensFirst*)sens_descs, sens_nz, B, H, W, desc.kernel_size, C, g, sens_part, sens_ticket, sens_sums));
    return DNNCA_OK;
}

// ---------------------------------------------------------------------------------------------- integrated gradients
// attr[b, h, w, c] = (x - x0) (1 / m) sum over k of d F_b / d x at x0 + alpha_k (x - x0), alpha_k = (k + 0.5) / m, F_b = sum over
// the image of sigmoid(logits_b), model in inference mode (include/dnnca.h).  Per step: the path input into a buffer of its own
// (x_dev is only read), sens_backward on it, and k_attr_first adds the signed first-layer dx into the accumulator -- step 0 stores,
// the later ones add, in ascending k, one writer per element: bit-identical from run to run.  Then attr_finish, and two more
// forwards (alpha = 0, then alpha = 1 on x_dev itself: the pass ends with the tensors and the input pointers of a forward of x_dev).
// Results: attr_out = [B, C, 2] (signed, absolute), then B x F(x), then B x F(x0); with want_map attr_acc holds attr.
int Model::integrated_gradients(const float* x_dev, int B, int steps, int baseline, bool want_map) {
    DN_TRY(sens_refusal("integrated gradients"));
    if (B < 1 || B > desc.max_batch) { set_error("batch %d outside [1, max_batch=%d]", B, desc.max_batch); return DNNCA_EINVAL; }
    if (steps < 1 || steps > kAttrMaxSteps) { set_error("integrated gradients: steps %d outside [1, %d]", steps, kAttrMaxSteps); return DNNCA_EINVAL; }
    if (baseline != 0 && baseline != 1) { set_error("integrated gradients: baseline %d is neither 0 (black) nor 1 (slice mean)", baseline); return DNNCA_EINVAL; }
    const int C = desc.in_channels, H = desc.height, W = desc.width;
    if (C > kAttrMaxC) { set_error("integrated gradients: %d input channels above %d", C, kAttrMaxC); return DNNCA_EINVAL; }
    const size_t hw = (size_t)H * W, hw_out = (size_t)outH * outW;
    if (!attr_acc) {
        const size_t mb = (size_t)desc.max_batch, nb = (size_t)std::max(attr_blocks(hw), attr_blocks(hw_out));
        DN_TRY(alloc((void**)&attr_acc, mb * hw * C * 4));
        DN_TRY(alloc((void**)&attr_in, mb * hw * C * 4));
        DN_TRY(alloc((void**)&attr_x0, mb * C * 4));
        DN_TRY(alloc((void**)&attr_part, mb * C * 2 * nb * 8));
        DN_TRY(alloc((void**)&attr_out, mb * (2 * C + 2) * 8));
    }
    attr_steps_last = steps;
    attr_baseline_last = baseline;
    const double xb = 4.0 * B * hw * C;
    const float* x0 = nullptr;
    if (baseline == 1) {
        LAUNCH(this, "attr_baseline_part", xb, (double)B * hw * C, g_attr_baseline_part(stream, x_dev, B, hw, C, attr_part));
        LAUNCH(this, "attr_baseline", 8.0 * B * C * attr_blocks(hw), (double)B * C * attr_blocks(hw),
               g_attr_baseline(stream, attr_part, B, hw, C, attr_x0));
        x0 = attr_x0;
    }
    double fb = 0, ff = 0;
    sens_first_cost(B, &fb, &ff);
    for (int k = 0; k < steps; ++k) {
        const float alpha = (float)(((double)k + 0.5) / (double)steps);
        LAUNCH(this, "attr_path_in", 2 * xb, 2.0 * B * hw * C, g_attr_path_in(stream, x_dev, x0, alpha, B, hw, C, attr_in));
        DN_TRY(sens_backward(attr_in, B));
        const SensFirstGrid g = sens_first_grid(B, H, W, sens_nz);
        LAUNCH(this, "attr_first", fb + (k ? 2 : 1) * xb, ff,
               g_attr_first(stream, (const SensFirst*)sens_descs, sens_nz, B, H, W, desc.kernel_size, C, g, attr_acc, k == 0));
    }
    const int nb = attr_blocks(hw), nbo = attr_blocks(hw_out);
    LAUNCH(this, "attr_finish", (want_map ? 3 : 2) * xb, 4.0 * B * hw * C,
           g_attr_finish(stream, attr_acc, x_dev, x0, steps, B, hw, C, want_map ? 1 : 0, attr_part));
    LAUNCH(this, "attr_sums", 8.0 * B * C * 2 * nb, (double)B * C * 2 * nb, g_attr_sums(stream, attr_part, B * C * 2, nb, attr_out));
    // the endpoints: F(x0) first, F(x) last
    for (int e = 1; e >= 0; --e) {
        const float* xe = x_dev;
        if (e == 1) {
            LAUNCH(this, "attr_base_in", 2 * xb, 2.0 * B * hw * C, g_attr_path_in(stream, x_dev, x0, 0.f, B, hw, C, attr_in));
            xe = attr_in;
        }
        sens_pass = true;
        const int frc = forward(xe, B, false);
        sens_pass = false;
        DN_TRY(frc);
        cur_op = nullptr;
        LAUNCH(this, "attr_prob_part", 4.0 * B * hw_out, 20.0 * B * hw_out, g_attr_prob_part(stream, dlogits, B, hw_out, attr_part));
        // row b of the [B, nbo] table -> entry b of endpoint e's run behind the [B, C, 2] sums
        LAUNCH(this, "attr_prob_sum", 8.0 * B * nbo, (double)B * nbo,
               g_attr_sums(stream, attr_part, B, nbo, attr_out + (size_t)B * C * 2 + (size_t)e * B));
    }
    return DNNCA_OK;
}

// [lo, hi) of the flat gradient vector is final on `stream`: sum it over the ranks on the communication stream
int Model::send_bucket(int64_t lo, int64_t hi) {
    if (hi <= lo) return DNNCA_OK;
    if (!comm_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&comm_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ev_bucket, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_comm_done, hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(ev_bucket, stream));
    HIP_TRY(hipStreamWaitEvent(comm_stream, ev_bucket, 0));
    if (step.wg_pending) {          // weight gradients of the bucket's layers may still be running on the side stream (FIFO: one event covers them)
        HIP_TRY(hipEventRecord(wg_bucket, wg_stream));
        HIP_TRY(hipStreamWaitEvent(comm_stream, wg_bucket, 0));
    }
    ncclResult_t r = ncclAllReduce(g + lo, g + lo, (size_t)(hi - lo), ncclFloat, ncclSum, comm, comm_stream);
    if (r != ncclSuccess) { set_error("ncclAllReduce(bucket): %s", ncclGetErrorString(r)); return DNNCA_ECOMM; }
    ++collectives_last_step;
    collective_floats_last_step = hi - lo;
    return DNNCA_OK;
}

// d_n = min(decay, (1 + n) / (10 + n)) with warm-up, decay without, in double; the kernels take (float)(1 - d_n) (as lr_t is made)
float Model::ema_next_om() {
    const int64_t n = dry ? ema.num_updates + 1 : ++ema.num_updates;
    double d = (double)ema.decay;
    if (ema.warmup) d = std::min(d, (1.0 + (double)n) / (10.0 + (double)n));
    return (float)(1.0 - d);
}

int Model::ema_refuse(const char* what) {
    if (!ema.in_use) return DNNCA_OK;
    set_error("%s: the averaged weights are in use (dnnca_ema_exchange): exchange back first", what);
    return DNNCA_ESTATE;
}

// the launches of a set optimizer (Model::opt): the norm of the gradient the optimizer receives and the clip scales, when a clip by
// norm is on, then the one pass that applies the update -- and, on a single replica, writes the step outputs
int Model::opt_launches(const float* grad, float lr, float lr_t, float gscale, float om) {
    const dnnca_optimizer_cfg& c = opt.cfg;
    if (opt.norm_clip()) {
        LAUNCH(this, "grad_sqnorm", 4.0 * nT, 3.0 * nT, g_grad_sqnorm(stream, opt.chunks, opt.nchunks, grad, gscale, c.clipvalue, opt.partials));
        LAUNCH(this, "grad_clip_scale", 16.0 * opt.nchunks, 2.0 * opt.nchunks,
               g_grad_clip_scale(stream, opt.var_first, opt.nvars, opt.nchunks, opt.partials, c.clipnorm, c.global_clipnorm, opt.scales,
                                 opt.norms));
    }
    OptArgs a{};
    a.lr_t = lr_t;
    a.lr = lr;
    a.lrwd = (float)((double)lr * (double)c.weight_decay);
    a.b1 = beta1; a.b2 = beta2; a.eps = eps;
    a.momentum = c.momentum;
    a.nesterov = c.nesterov;
    a.gscale = gscale;
    a.clipvalue = c.clipvalue;
    a.scales = opt.norm_clip() ? opt.scales : nullptr;
    a.om = om;
    AdamFinalize fin{};
    if (step.fin_pending.on) {
        step.fin_pending.on = false;          // consumed: this launch writes the step outputs
        fin = AdamFinalize{scalars, step.fin_pending.cfg, step.fin_pending.n_label, step.fin_pending.inv_batch_hw, out5};
    }
    // bytes per parameter: p and g read, p written, and the slots the kind touches (m, v read and written); the average adds 8
    const bool sgd = c.kind == DNNCA_OPT_SGD;
    const double per = (sgd ? (c.momentum == 0.f ? 12.0 : 20.0) : 28.0) + (ema.e ? 8.0 : 0.0);
    const double fl = (sgd ? 4.0 : (c.kind == DNNCA_OPT_ADAMW ? 12.0 : 10.0)) + (ema.e ? 3.0 : 0.0);
    static const char* const names[3][2] = {{"opt_adam", "opt_adam_ema"}, {"opt_adamw", "opt_adamw_ema"}, {"opt_sgd", "opt_sgd_ema"}};
    LAUNCH(this, names[c.kind][ema.e ? 1 : 0], per * nT, fl * nT,
           g_opt_step(stream, c.kind, opt.chunks, opt.nchunks, p, grad, m, v, ema.e, a, fin));
    return DNNCA_OK;
}

// Gradient accumulation, the first part of optimizer_step while accum.a: this micro-step's gradient goes into the accumulator
// (grad_accumulate, unless the deferred fold takes it along: pg_fold_acc), and under a communicator the reduction follows on the
// model's stream: the loss slot alone on a micro-step that ends in no update (the reported loss stays the cross-replica mean), the
// accumulator with the loss slot behind it on the one that does.  Moves accum.pos (never in a dry plan run).  Returns with
// accum.pos == 0 when the update is due
int Model::accumulate(bool reduce) {
    const int j = accum.pos + 1;                       // this micro-step's place in the cycle, 1 .. steps
    const bool last = j == accum.steps, first = j == 1;
    const bool reduces = reduce && comm && !dry;
    if (step.fold_deferred) {
        if (!step.fin_pending.on || last) { set_error("internal: deferred gradient fold without an accumulating micro-step"); return DNNCA_ESTATE; }
        step.fin_pending.on = false;          // consumed: this launch writes the step outputs
        DN_TRY(fast_fold_acc(this, first, step.fin_pending.cfg, step.fin_pending.n_label, step.fin_pending.inv_batch_hw));
    } else {
        AdamFinalize fin{};
        if (!last && step.fin_pending.on) {      // no optimizer launch follows: this one writes the step outputs
            step.fin_pending.on = false;
            fin = AdamFinalize{scalars, step.fin_pending.cfg, step.fin_pending.n_label, step.fin_pending.inv_batch_hw, out5};
        }
        // bytes per parameter: g read and a written; a read as well once the cycle has begun
        LAUNCH(this, "grad_accumulate", (first ? 8.0 : 12.0) * nT, (first ? 0.0 : 1.0) * nT,
               g_grad_accumulate(stream, (size_t)nT, accum.a, g, first, fin, reduces && last));
    }
    if (reduces) {
        // the loss slot travels as a[nT] on the update micro-step: one all-reduce over [accumulated gradients ..., loss]
        float* buf = last ? accum.a : out5;
        const size_t count = last ? (size_t)nT + 1 : 1;
        ncclResult_t r = ncclAllReduce(buf, buf, count, ncclFloat, ncclSum, comm, stream);
        if (r != ncclSuccess) { set_error("ncclAllReduce(accumulation): %s", ncclGetErrorString(r)); return DNNCA_ECOMM; }
        collectives_last_step = 1;
        collective_floats_last_step = (int64_t)count;
        if (last) HIP_TRY(hipMemcpyAsync(out5, accum.a + nT, 4, hipMemcpyDeviceToDevice, stream));
    }
    if (!dry) accum.pos = last ? 0 : j;
    return DNNCA_OK;
}

// reduce == false (dnnca_apply_gradients): the gradient vector is taken as it stands, without a communicator
int Model::optimizer_step(float lr, bool reduce) {
    cur_op = nullptr;
    float gscale = 1.0f;
    const float* grad = g;          // what the optimizer receives: this step's gradient, or the accumulator at the end of a cycle
    if (accum.a) {
        const bool last = accum.pos + 1 == accum.steps;
        DN_TRY(accumulate(reduce));
        if (!last) return DNNCA_OK;          // nothing else changes: weights, slots, iterations and the weight average stay
        grad = accum.a;
        gscale = (float)(1.0 / ((double)accum.steps * (double)(reduce && comm && !dry ? world : 1)));      // the mean, rounded once
    } else if (reduce && comm && !dry && step.bucketing) {
        // the backward pass has sent the finalised suffix in buckets; what is left -- the first layers and the step's loss in the
        // tail -- follows on the same (communication) stream, and Adam waits for all of it
        step.bucketing = false;
        DN_TRY(send_bucket(0, step.bucket_hi));
        DN_TRY(send_bucket(nT, nT + 1));
        HIP_TRY(hipEventRecord(ev_comm_done, comm_stream));
        HIP_TRY(hipStreamWaitEvent(stream, ev_comm_done, 0));
        gscale = 1.0f / (float)world;
    } else if (reduce && comm && !dry) {
        // one all-reduce over [gradients ..., loss]: MirroredStrategy's cross-replica sum (engine.py:262) [TF-2.6]
        ncclResult_t r = ncclAllReduce(g, g, (size_t)nT + 1, ncclFloat, ncclSum, comm, stream);
        if (r != ncclSuccess) { set_error("ncclAllReduce: %s", ncclGetErrorString(r)); return DNNCA_ECOMM; }
        collectives_last_step = 1;
        collective_floats_last_step = nT + 1;
        gscale = 1.0f / (float)world;
    }
    iterations += dry ? 0 : 1;
    double t = (double)(dry ? 1 : iterations);
    float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)beta2, t)) / (1.0 - std::pow((double)beta1, t)));
    const float om = ema.e ? ema_next_om() : 0.f;          // the weight average rides whichever Adam launch runs
    if (step.fin_pending.on && step.fold_deferred) {
        step.fin_pending.on = false;          // consumed (here and below): this launch writes the step outputs
        return fast_fold_adam(this, lr_t, om, step.fin_pending.cfg, step.fin_pending.n_label, step.fin_pending.inv_batch_hw);
    }
    if (step.fold_deferred) { set_error("internal: deferred gradient fold without a single-replica optimizer step"); return DNNCA_ESTATE; }
    if (opt.on) return opt_launches(grad, lr, lr_t, gscale, om);
    if (step.fin_pending.on) {
        step.fin_pending.on = false;
        if (ema.e) {
            LAUNCH(this, "g_adam_ema", 36.0 * nT, 13.0 * nT,
                   g_adam_finalize(stream, (size_t)nT, p, grad, m, v, lr_t, beta1, beta2, eps, gscale, scalars, step.fin_pending.cfg,
                                   step.fin_pending.n_label, step.fin_pending.inv_batch_hw, out5, ema.e, om));
            return DNNCA_OK;
        }
        LAUNCH(this, "g_adam", 28.0 * nT, 10.0 * nT,
               g_adam_finalize(stream, (size_t)nT, p, grad, m, v, lr_t, beta1, beta2, eps, gscale, scalars, step.fin_pending.cfg,
                               step.fin_pending.n_label, step.fin_pending.inv_batch_hw, out5));
        return DNNCA_OK;
    }
    if (ema.e) {
        LAUNCH(this, "g_adam_ema", 36.0 * nT, 13.0 * nT, g_adam(stream, (size_t)nT, p, grad, m, v, lr_t, beta1, beta2, eps, gscale, ema.e, om));
        return DNNCA_OK;
    }
    LAUNCH(this, "g_adam", 28.0 * nT, 10.0 * nT, g_adam(stream, (size_t)nT, p, grad, m, v, lr_t, beta1, beta2, eps, gscale));
    return DNNCA_OK;
}

}  // namespace dnnca

// =================================================================================================== C ABI
// (test-time augmentation and the analysis entry points -- confusion, region metrics, lesion tables, boundary distances, spread,
// calibration -- are in abi_analysis.hip)
using namespace dnnca;

extern "C" {

const char* dnnca_version(void) { return "dnnca 0.1 (gfx950)"; }
const char* dnnca_last_error(void) { return g_err; }

int dnnca_device_count(int* count) {
    if (!count) return DNNCA_EINVAL;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return DNNCA_EHIP; }
    *count = n;
    return DNNCA_OK;
}

int dnnca_init(int device_ordinal) {
    HIP_TRY(hipSetDevice(device_ordinal));
    return DNNCA_OK;
}

int dnnca_model_create(const dnnca_model_desc* desc, void** model_out) {
    if (!desc || !model_out) { set_error("null argument"); return DNNCA_EINVAL; }
    *model_out = nullptr;
    Model* M = new Model();
    M->desc = *desc;
    if (M->desc.n_conv == 0) M->desc.n_conv = 2;
    hipError_t e = hipGetDevice(&M->device);
    if (e != hipSuccess) { set_error("no HIP device: %s", hipGetErrorString(e)); delete M; return DNNCA_EHIP; }
    e = hipStreamCreateWithFlags(&M->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { set_error("hipStreamCreate: %s", hipGetErrorString(e)); M->stream = nullptr; delete M; return DNNCA_EHIP; }
    int rc = M->build();
    if (rc != DNNCA_OK) { delete M; return rc; }
    *model_out = M;
    return DNNCA_OK;
}

int dnnca_model_destroy(void* model) {
    MODEL(model);
    (void)hipStreamSynchronize(M->stream);
    delete M;
    return DNNCA_OK;
}

int dnnca_param_count(void* model, int* count) {
    MODEL(model);
    *count = (int)M->params.size();
    return DNNCA_OK;
}

int dnnca_param_info(void* model, int index, char* name, size_t name_cap, int64_t shape[4], int* ndim, int* trainable,
                     int64_t* offset) {
    MODEL(model);
    if (index < 0 || index >= (int)M->params.size()) { set_error("param index out of range"); return DNNCA_EINVAL; }
    const ParamInfo& pi = M->params[index];
    if (name && name_cap) snprintf(name, name_cap, "%s", pi.name.c_str());
    if (shape) for (int i = 0; i < 4; ++i) shape[i] = pi.shape[i];
    if (ndim) *ndim = pi.ndim;
    if (trainable) *trainable = pi.trainable;
    if (offset) *offset = pi.offset;
    return DNNCA_OK;
}

int dnnca_num_trainable(void* model, int64_t* n) { MODEL(model); *n = M->nT; return DNNCA_OK; }
int dnnca_num_state(void* model, int64_t* n) { MODEL(model); *n = M->nS; return DNNCA_OK; }

static int copy_flat(Model* M, float* dev, int64_t have, const float* src, float* dst, int64_t n) {
    if (n != have) { set_error("flat vector length %lld != %lld", (long long)n, (long long)have); return DNNCA_EINVAL; }
    if (n == 0) return DNNCA_OK;
    if (src) HIP_TRY(hipMemcpyAsync(dev, src, (size_t)n * 4, hipMemcpyHostToDevice, M->stream));
    if (dst) HIP_TRY(hipMemcpyAsync(dst, dev, (size_t)n * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

int dnnca_set_params(void* model, const float* flat, int64_t n) {
    MODEL(model);
    DN_TRY(M->ema_refuse("dnnca_set_params"));
    DN_TRY(copy_flat(M, M->p, M->nT, flat, nullptr, n));
    M->accum.pos = 0;          // new weights: a partial cycle of gradients taken at the old ones is dropped
    return DNNCA_OK;
}
int dnnca_get_params(void* model, float* flat, int64_t n) { MODEL(model); return copy_flat(M, M->p, M->nT, nullptr, flat, n); }
int dnnca_set_state(void* model, const float* flat, int64_t n) { MODEL(model); return copy_flat(M, M->state, M->nS, flat, nullptr, n); }
int dnnca_get_state(void* model, float* flat, int64_t n) { MODEL(model); return copy_flat(M, M->state, M->nS, nullptr, flat, n); }
int dnnca_get_grads(void* model, float* flat, int64_t n) { MODEL(model); return copy_flat(M, M->g, M->nT, nullptr, flat, n); }

int dnnca_set_opt_state(void* model, const float* m, const float* v, int64_t n, int64_t iterations) {
    MODEL(model);
    DN_TRY(M->ema_refuse("dnnca_set_opt_state"));
    DN_TRY(copy_flat(M, M->m, M->nT, m, nullptr, n));
    DN_TRY(copy_flat(M, M->v, M->nT, v, nullptr, n));
    M->iterations = iterations;
    M->accum.pos = 0;
    return DNNCA_OK;
}

int dnnca_get_opt_state(void* model, float* m, float* v, int64_t n, int64_t* iterations) {
    MODEL(model);
    DN_TRY(copy_flat(M, M->m, M->nT, nullptr, m, n));
    DN_TRY(copy_flat(M, M->v, M->nT, nullptr, v, n));
    if (iterations) *iterations = M->iterations;
    return DNNCA_OK;
}

// ---- exponential moving average of the weights (Model::ema) -------------------------------------------------------------------
int dnnca_model_set_ema(void* model, float decay, int warmup) {
    MODEL(model);
    DN_TRY(M->ema_refuse("dnnca_model_set_ema"));
    if (!(decay == 0.f || (decay > 0.f && decay < 1.f))) { set_error("dnnca_model_set_ema: decay %g outside (0, 1) (0 switches it off)", (double)decay); return DNNCA_EINVAL; }
    HIP_TRY(hipStreamSynchronize(M->stream));
    if (decay == 0.f) {
        if (M->ema.e) HIP_TRY(hipFree(M->ema.e));
        M->ema = Model::Ema{};
        return DNNCA_OK;
    }
    if (!M->ema.e) HIP_TRY(hipMalloc((void**)&M->ema.e, (size_t)(M->nT + 4) * 4));
    HIP_TRY(hipMemcpyAsync(M->ema.e, M->p, (size_t)M->nT * 4, hipMemcpyDeviceToDevice, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    M->ema.decay = decay;
    M->ema.warmup = warmup != 0;
    M->ema.num_updates = 0;
    return DNNCA_OK;
}

static int ema_required(Model* M, const char* what) {
    if (M->ema.e) return DNNCA_OK;
    set_error("%s: no weight average (dnnca_model_set_ema)", what);
    return DNNCA_ESTATE;
}

int dnnca_get_ema(void* model, float* flat, int64_t n, int64_t* num_updates) {
    MODEL(model);
    DN_TRY(ema_required(M, "dnnca_get_ema"));
    if (flat) DN_TRY(copy_flat(M, M->ema.e, M->nT, nullptr, flat, n));
    if (num_updates) *num_updates = M->ema.num_updates;
    return DNNCA_OK;
}

int dnnca_set_ema_state(void* model, const float* flat, int64_t n, int64_t num_updates) {
    MODEL(model);
    DN_TRY(ema_required(M, "dnnca_set_ema_state"));
    DN_TRY(M->ema_refuse("dnnca_set_ema_state"));
    if (!flat || num_updates < 0) { set_error("dnnca_set_ema_state: null vector or negative num_updates"); return DNNCA_EINVAL; }
    DN_TRY(copy_flat(M, M->ema.e, M->nT, flat, nullptr, n));
    M->ema.num_updates = num_updates;
    return DNNCA_OK;
}

int dnnca_ema_exchange(void* model) {
    MODEL(model);
    DN_TRY(ema_required(M, "dnnca_ema_exchange"));
    M->cur_op = nullptr;
    LAUNCH(M, "ema_exchange", 16.0 * M->nT, 0, g_ema_exchange(M->stream, (size_t)M->nT, M->p, M->ema.e));
    M->ema.in_use = !M->ema.in_use;
    return DNNCA_OK;
}

int dnnca_set_adam(void* model, float beta1, float beta2, float epsilon) {
    MODEL(model);
    M->beta1 = beta1;
    M->beta2 = beta2;
    M->eps = epsilon;
    return DNNCA_OK;
}

// ---- configurable optimizers (Model::opt, optim.h) ----------------------------------------------------------------------------
static int opt_bad(const char* what, double value, const char* want) {
    set_error("dnnca_model_set_optimizer: %s %g: %s", what, value, want);
    return DNNCA_EINVAL;
}

int dnnca_model_set_optimizer(void* model, const dnnca_optimizer_cfg* cfg, const uint8_t* decay_per_variable, int n_variables) {
    MODEL(model);
    DN_TRY(M->ema_refuse("dnnca_model_set_optimizer"));
    if (!cfg) { set_error("dnnca_model_set_optimizer: null cfg"); return DNNCA_EINVAL; }
    const dnnca_optimizer_cfg c = *cfg;
    if (c.kind != DNNCA_OPT_ADAM && c.kind != DNNCA_OPT_ADAMW && c.kind != DNNCA_OPT_SGD) return opt_bad("kind", c.kind, "not one of DNNCA_OPT_ADAM / ADAMW / SGD");
    const bool sgd = c.kind == DNNCA_OPT_SGD;
    if (!sgd) {
        if (!(c.beta1 >= 0.f && c.beta1 < 1.f)) return opt_bad("beta_1", c.beta1, "must lie in [0, 1)");
        if (!(c.beta2 >= 0.f && c.beta2 < 1.f)) return opt_bad("beta_2", c.beta2, "must lie in [0, 1)");
        if (!(c.epsilon >= 0.f && std::isfinite(c.epsilon))) return opt_bad("epsilon", c.epsilon, "must be finite and >= 0");
    }
    if (!(c.momentum >= 0.f && c.momentum < 1.f)) return opt_bad("momentum", c.momentum, "must lie in [0, 1)");
    if (!(c.weight_decay >= 0.f && std::isfinite(c.weight_decay))) return opt_bad("weight_decay", c.weight_decay, "must be finite and >= 0");
    if (c.nesterov != 0 && c.nesterov != 1) return opt_bad("nesterov", c.nesterov, "must be 0 or 1");
    if (!sgd && (c.momentum != 0.f || c.nesterov)) return opt_bad("momentum", c.momentum, "momentum / nesterov belong to DNNCA_OPT_SGD");
    if (c.kind != DNNCA_OPT_ADAMW && c.weight_decay != 0.f) return opt_bad("weight_decay", c.weight_decay, "belongs to DNNCA_OPT_ADAMW");
    const struct { const char* name; float v; } clips[3] = {{"clipvalue", c.clipvalue}, {"clipnorm", c.clipnorm}, {"global_clipnorm", c.global_clipnorm}};
    for (const auto& k : clips)
        if (!(k.v >= 0.f && std::isfinite(k.v))) return opt_bad(k.name, k.v, "must be finite and > 0 (0: off)");
    if (c.clipnorm > 0.f && c.global_clipnorm > 0.f) return opt_bad("clipnorm", c.clipnorm, "clipnorm and global_clipnorm exclude each other");
    int nvars = 0;
    for (const ParamInfo& pi : M->params) nvars += pi.trainable ? 1 : 0;
    const bool plain = c.kind == DNNCA_OPT_ADAM && c.clipvalue == 0.f && c.clipnorm == 0.f && c.global_clipnorm == 0.f;
    if (!plain && n_variables != nvars) return opt_bad("n_variables", n_variables, "is not the number of trainable variables");
    if (c.kind == DNNCA_OPT_ADAMW && !decay_per_variable) { set_error("dnnca_model_set_optimizer: DNNCA_OPT_ADAMW without decay_per_variable"); return DNNCA_EINVAL; }
    if (M->nT >= (int64_t)1 << 31) { set_error("dnnca_model_set_optimizer: %lld parameters do not fit the chunk table", (long long)M->nT); return DNNCA_EINVAL; }
    HIP_TRY(hipStreamSynchronize(M->stream));
    if (!sgd) { M->beta1 = c.beta1; M->beta2 = c.beta2; M->eps = c.epsilon; }
    if (M->opt.table) HIP_TRY(hipFree(M->opt.table));
    M->opt = Model::Optim{};
    if (plain) return DNNCA_OK;
    // the chunk table: fixed-size chunks, none straddling a variable, each with its variable's index and decay flag
    std::vector<OptChunk> chunks;
    std::vector<int> var_first;
    int v = 0;
    for (const ParamInfo& pi : M->params) {
        if (!pi.trainable) continue;
        var_first.push_back((int)chunks.size());
        const int decay = c.kind == DNNCA_OPT_ADAMW && decay_per_variable[v] ? 1 : 0;
        for (int64_t lo = 0; lo < pi.size; lo += kOptChunk)
            chunks.push_back(OptChunk{(int)(pi.offset + lo), (int)std::min<int64_t>(kOptChunk, pi.size - lo), v, decay});
        ++v;
    }
    var_first.push_back((int)chunks.size());
    Model::Optim& o = M->opt;
    o.nchunks = (int)chunks.size();
    o.nvars = nvars;
    // doubles first (8-byte aligned), then the 16-byte chunks, then ints and floats
    const size_t b_part = (size_t)o.nchunks * 8, b_norm = (size_t)(1 + nvars) * 8, b_chunk = (size_t)o.nchunks * sizeof(OptChunk);
    const size_t b_first = (size_t)(nvars + 1) * 4, b_scale = (size_t)nvars * 4;
    const size_t pad = (16 - (b_part + b_norm) % 16) % 16;
    HIP_TRY(hipMalloc(&o.table, b_part + b_norm + pad + b_chunk + b_first + b_scale));
    char* base = (char*)o.table;
    o.partials = (double*)base;
    o.norms = (double*)(base + b_part);
    o.chunks = (OptChunk*)(base + b_part + b_norm + pad);
    o.var_first = (int*)(base + b_part + b_norm + pad + b_chunk);
    o.scales = (float*)(base + b_part + b_norm + pad + b_chunk + b_first);
    HIP_TRY(hipMemsetAsync(o.table, 0, b_part + b_norm, M->stream));
    HIP_TRY(hipMemcpyAsync(o.chunks, chunks.data(), b_chunk, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipMemcpyAsync(o.var_first, var_first.data(), b_first, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));          // the tables are locals
    o.cfg = c;
    o.on = true;
    return DNNCA_OK;
}

int dnnca_last_grad_norm(void* model, double* global, double* per_variable, int n) {
    MODEL(model);
    if (!M->opt.norm_clip()) { set_error("dnnca_last_grad_norm: no clipping by norm is set (dnnca_model_set_optimizer)"); return DNNCA_ESTATE; }
    if (n != 0 && n != M->opt.nvars) { set_error("dnnca_last_grad_norm: n %d is neither 0 nor the %d trainable variables", n, M->opt.nvars); return DNNCA_EINVAL; }
    std::vector<double> h((size_t)1 + M->opt.nvars);
    HIP_TRY(hipMemcpyAsync(h.data(), M->opt.norms, h.size() * 8, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    if (global) *global = h[0];
    if (per_variable && n) memcpy(per_variable, h.data() + 1, (size_t)n * 8);
    return DNNCA_OK;
}

int dnnca_apply_gradients(void* model, const float* g_host, int64_t n, float lr) {
    MODEL(model);
    DN_TRY(M->ema_refuse("dnnca_apply_gradients"));
    if (!g_host || n != M->nT) { set_error("dnnca_apply_gradients: null vector or %lld elements for %lld trainable parameters", (long long)n, (long long)M->nT); return DNNCA_EINVAL; }
    M->step = Model::Step{};          // no pass is under way: nothing is pending, nothing deferred
    HIP_TRY(hipMemcpyAsync(M->g, g_host, (size_t)n * 4, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));          // the caller's vector may be reused at once
    return M->optimizer_step(lr, false);
}

// ---- gradient accumulation (Model::accum, accum.h) ----------------------------------------------------------------------------
int dnnca_model_set_accumulation(void* model, int steps) {
    MODEL(model);
    if (steps < 1 || steps > kAccumMaxSteps) { set_error("dnnca_model_set_accumulation: steps %d outside [1, %d]", steps, kAccumMaxSteps); return DNNCA_EINVAL; }
    DN_TRY(M->ema_refuse("dnnca_model_set_accumulation"));
    HIP_TRY(hipStreamSynchronize(M->stream));
    if (steps == 1) {
        if (M->accum.a) HIP_TRY(hipFree(M->accum.a));
        M->accum = Model::Accum{};
        return DNNCA_OK;
    }
    if (!M->accum.a) {
        // nT floats, the loss slot behind them, padding to whole float4s; zeroed: readable before the first micro-step
        HIP_TRY(hipMalloc((void**)&M->accum.a, (size_t)(M->nT + 4) * 4));
        HIP_TRY(hipMemsetAsync(M->accum.a, 0, (size_t)(M->nT + 4) * 4, M->stream));
        HIP_TRY(hipStreamSynchronize(M->stream));
    }
    M->accum.steps = steps;
    M->accum.pos = 0;          // a partial cycle is discarded: the next micro-step starts one (a <- g)
    return DNNCA_OK;
}

int dnnca_get_accumulation(void* model, float* flat, int64_t n, int* steps, int* position) {
    MODEL(model);
    if (!M->accum.a) { set_error("dnnca_get_accumulation: gradient accumulation is off (dnnca_model_set_accumulation)"); return DNNCA_ESTATE; }
    if (flat) DN_TRY(copy_flat(M, M->accum.a, M->nT, nullptr, flat, n));
    else HIP_TRY(hipStreamSynchronize(M->stream));
    if (steps) *steps = M->accum.steps;
    if (position) *position = M->accum.pos;
    return DNNCA_OK;
}

int dnnca_grad_accumulate_of(void* model, const float* acc_host, const float* g_host, int64_t n, int first, float* out_host) {
    MODEL(model);
    if (n < 1 || n >= (int64_t)1 << 40) { set_error("dnnca_grad_accumulate_of: %lld elements", (long long)n); return DNNCA_EINVAL; }
    if (!g_host || !out_host || (!first && !acc_host)) { set_error("dnnca_grad_accumulate_of: null buffer"); return DNNCA_EINVAL; }
    float* dev = nullptr;          // [a | g], each n + 4 floats: whole float4s and the (unused) loss slot
    const size_t row = (size_t)n + 4;
    HIP_TRY(hipMalloc((void**)&dev, 2 * row * 4));
    hipError_t e = hipSuccess;
    if (!first) e = hipMemcpyAsync(dev, acc_host, (size_t)n * 4, hipMemcpyHostToDevice, M->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + row, g_host, (size_t)n * 4, hipMemcpyHostToDevice, M->stream);
    if (e == hipSuccess) {
        g_grad_accumulate(M->stream, (size_t)n, dev, dev + row, first != 0, AdamFinalize{}, false);
        e = hipMemcpyAsync(out_host, dev, (size_t)n * 4, hipMemcpyDeviceToHost, M->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(M->stream);
    (void)hipFree(dev);
    if (e != hipSuccess) { set_error("dnnca_grad_accumulate_of: %s", hipGetErrorString(e)); return DNNCA_EHIP; }
    return DNNCA_OK;
}

}  // extern "C"

// ---- helpers of the step entry points (those without `static` are declared in abi.h) -----------------------------------------
namespace dnnca {

// a host batch -> x_stage and, with `labels`, y_stage
int stage_inputs(Model* M, int batch, const float* x_nhwc, const float* y_hw, bool labels) {
    DN_TRY(check_batch(M, batch));
    const size_t nx = (size_t)batch * M->desc.height * M->desc.width * M->desc.in_channels;
    const size_t npix = (size_t)batch * M->outH * M->outW;
    HIP_TRY(hipMemcpyAsync(M->x_stage, x_nhwc, nx * 4, hipMemcpyHostToDevice, M->stream));
    if (labels) HIP_TRY(hipMemcpyAsync(M->y_stage, y_hw, npix * 4, hipMemcpyHostToDevice, M->stream));
    return DNNCA_OK;
}

// h: the five step outputs; ranks: how many ranks' local means the loss slot holds the sum of (train steps are all-reduced:
// the world size; evaluation is rank-local: 1)
static int convert_out(const float* h, int ranks, dnnca_step_out* out) {
    out->loss = h[0] / (float)ranks;
    out->positive_rate = h[1];
    out->weight = h[2];
    out->label_min = h[3];
    out->label_max = h[4];
    // utils/losses.py:91-92 assert_on_max / assert_on_min, :30 assert_on_weight
    if (h[4] > 1.0f || h[3] < 0.0f) { set_error("label outside [0, 1]: min %g max %g (assert_on_min/assert_on_max)", h[3], h[4]); return DNNCA_EASSERT; }
    if (h[2] < 0.0f) { set_error("negative class weight %g (assert_on_weight)", h[2]); return DNNCA_EASSERT; }
    return DNNCA_OK;
}

static int read_out(Model* M, int ranks, dnnca_step_out* out) {
    float h[5];
    HIP_TRY(hipMemcpyAsync(h, M->out5, sizeof(h), hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    DN_TRY(M->flush_profile());
    return convert_out(h, ranks, out);
}

// ---- pixel confusion: one threshold table type, one histogram kernel (g_conf_hist) -------------------------------------------
static int check_thresholds(const float* thresholds, int n) {
    if (n < 0 || n > DNNCA_CONF_MAX_THR || (n > 0 && !thresholds)) { set_error("bad thresholds (0..%d)", DNNCA_CONF_MAX_THR); return DNNCA_EINVAL; }
    return DNNCA_OK;
}

// thresholds -> ascending in t.dev (the histogram kernel wants them sorted); t.order[i] = the caller's position of sorted i.
// Returns with the upload done; on an error the table is empty.
static int conf_thresholds_set(Model* M, ConfThresholds& t, const float* thresholds, int n) {
    t.n = 0;
    t.order.resize(n);
    if (n == 0) return DNNCA_OK;
    for (int i = 0; i < n; ++i) t.order[i] = i;
    std::stable_sort(t.order.begin(), t.order.end(), [&](int a, int b) { return thresholds[a] < thresholds[b]; });
    std::vector<float> sorted(n);
    for (int i = 0; i < n; ++i) {
        sorted[i] = thresholds[t.order[i]];
        if (sorted[i] != sorted[i]) { set_error("threshold %d is NaN", t.order[i]); return DNNCA_EINVAL; }
    }
    HIP_TRY(hipMemcpyAsync(t.dev, sorted.data(), (size_t)n * 4, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));          // `sorted` is a local
    t.n = n;
    return DNNCA_OK;
}

// histogram [positives | negatives][n + 1 bins] -> TP / FP / FN / TN per threshold, in the caller's order
static void confusion_from_hist(const unsigned long long* h, const ConfThresholds& t, dnnca_confusion* out) {
    const int n = t.n;
    const unsigned long long* pos = h;
    const unsigned long long* neg = h + (n + 1);
    unsigned long long P = 0, N = 0;
    for (int b = 0; b <= n; ++b) { P += pos[b]; N += neg[b]; }
    unsigned long long tp = 0, fp = 0;            // suffix sums: prob > sorted[t]  <=>  bin > t
    for (int i = n - 1; i >= 0; --i) {
        tp += pos[i + 1];
        fp += neg[i + 1];
        dnnca_confusion& o = out[t.order[i]];
        o.tp = (double)tp;
        o.fp = (double)fp;
        o.fn = (double)(P - tp);
        o.tn = (double)(N - fp);
    }
}

// evaluation and the one-shot counts: eval_thr + the histogram conf_dev, which keeps adding up until it is read
int confusion_begin(Model* M, const float* thresholds, int n) {
    DN_TRY(conf_thresholds_set(M, M->eval_thr, thresholds, n));
    HIP_TRY(hipMemsetAsync(M->conf_dev, 0, (size_t)2 * (n + 1) * 8, M->stream));
    return DNNCA_OK;
}

void confusion_add(Model* M, size_t npix, const float* y_dev) {
    g_conf_hist(M->stream, npix, M->prob, y_dev, M->eval_thr.dev, M->eval_thr.n, reinterpret_cast<unsigned long long*>(M->conf_dev),
                nullptr);
}

int confusion_finish(Model* M, dnnca_confusion* out) {
    std::vector<unsigned long long> h((size_t)2 * (M->eval_thr.n + 1));
    HIP_TRY(hipMemcpyAsync(h.data(), M->conf_dev, h.size() * 8, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    confusion_from_hist(h.data(), M->eval_thr, out);
    return DNNCA_OK;
}

// per-step training metrics: the step just enqueued, its probabilities (M->prob, written by the head) against its raw labels at
// tm_thr -> tm_hist[row] -> tm_pin[row]
static int train_metrics_count(Model* M, const float* y_dev, int batch, int row) {
    const size_t npix = (size_t)batch * M->outH * M->outW;
    const int n = M->tm_thr.n;
    unsigned long long* hist = M->tm_hist + (size_t)row * Model::kTmRow;
    LAUNCH(M, "train_conf_hist", 8.0 * npix, 10.0 * npix,
           g_conf_hist(M->stream, npix, M->prob, y_dev, M->tm_thr.dev, n, M->tm_scratch, hist));
    if (M->dry) return DNNCA_OK;
    HIP_TRY(hipMemcpyAsync(M->tm_pin + (size_t)row * Model::kTmRow, hist, (size_t)2 * (n + 1) * 8, hipMemcpyDeviceToHost, M->stream));
    M->tm_ran[row] = n;
    return DNNCA_OK;
}

}  // namespace dnnca

extern "C" {

// ---- steps on host or device batches ------------------------------------------------------------------------------------------
int dnnca_forward_dev(void* model, const float* x_dev, int batch, int training) {
    MODEL(model);
    DN_TRY(M->forward(x_dev, batch, training != 0));
    size_t npix = (size_t)batch * M->outH * M->outW;
    LAUNCH(M, "g_sigmoid", 8.0 * npix, 4.0 * npix, g_sigmoid(M->stream, npix, M->logits, M->prob));
    return DNNCA_OK;
}

int dnnca_forward(void* model, const float* x_nhwc, int batch, int training, float* prob_out, float* logit_out) {
    MODEL(model);
    DN_TRY(stage_inputs(M, batch, x_nhwc, nullptr, false));
    const size_t npix = (size_t)batch * M->outH * M->outW;
    DN_TRY(dnnca_forward_dev(model, M->x_stage, batch, training));
    if (prob_out) HIP_TRY(hipMemcpyAsync(prob_out, M->prob, npix * 4, hipMemcpyDeviceToHost, M->stream));
    if (logit_out) HIP_TRY(hipMemcpyAsync(logit_out, M->logits, npix * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return M->flush_profile();
}

// What a train step enqueues, for dnnca_train_step* and for the plan dump (dry): forward with the step's request, loss + backward,
// optimizer, the training-metric count.  row: the tm_hist / tm_pin row of the counts (the step's staging slot, or kStageSlots)
static int train_pass(Model* M, const float* x_dev, const float* y_dev, int batch, float lr, const dnnca_loss_cfg& cfg, int row) {
    const StepRequest req{y_dev, cfg, true, head_in_conv_requested(M, cfg)};
    DN_TRY(M->forward(x_dev, batch, true, req));
    DN_TRY(M->loss_and_backward(y_dev, batch, cfg, true));
    DN_TRY(M->optimizer_step(lr));
    if (!M->dry) M->tm_ran[row] = 0;
    if (M->train_metrics_on()) DN_TRY(train_metrics_count(M, y_dev, batch, row));      // the raw labels, never y_smooth
    return DNNCA_OK;
}

static int train_step_impl(Model* M, const float* x_dev, const float* y_dev, int batch, float lr, const dnnca_loss_cfg* cfg,
                           dnnca_step_out* out, int row) {
    if (!cfg) { set_error("null loss cfg"); return DNNCA_EINVAL; }
    DN_TRY(M->ema_refuse("train step"));
    DN_TRY(train_pass(M, x_dev, y_dev, batch, lr, *cfg, row));
    if (out) return read_out(M, M->world, out);      // after the all-reduce the loss slot holds the sum over ranks of the local means
    return DNNCA_OK;
}

int dnnca_train_step_dev(void* model, const float* x_dev, const float* y_dev, int batch, float lr, const dnnca_loss_cfg* cfg,
                         dnnca_step_out* out) {
    MODEL(model);
    return train_step_impl(M, x_dev, y_dev, batch, lr, cfg, out, Model::kStageSlots);
}

int dnnca_train_step(void* model, const float* x_nhwc, const float* y_hw, int batch, float lr, const dnnca_loss_cfg* cfg,
                     dnnca_step_out* out) {
    MODEL(model);
    DN_TRY(stage_inputs(M, batch, x_nhwc, y_hw, true));
    dnnca_step_out tmp;
    return dnnca_train_step_dev(model, M->x_stage, M->y_stage, batch, lr, cfg, out ? out : &tmp);
}

int dnnca_eval_step(void* model, const float* x_nhwc, const float* y_hw, int batch, const dnnca_loss_cfg* cfg,
                    dnnca_step_out* out, float* prob_out) {
    MODEL(model);
    if (!cfg) { set_error("null loss cfg"); return DNNCA_EINVAL; }
    DN_TRY(stage_inputs(M, batch, x_nhwc, y_hw, true));
    DN_TRY(M->forward(M->x_stage, batch, false));
    DN_TRY(M->loss_and_backward(M->y_stage, batch, *cfg, false));
    if (prob_out) HIP_TRY(hipMemcpyAsync(prob_out, M->prob, (size_t)batch * M->outH * M->outW * 4, hipMemcpyDeviceToHost, M->stream));
    dnnca_step_out tmp;
    return read_out(M, 1, out ? out : &tmp);         // evaluation is rank-local: the loss slot was not all-reduced
}

int dnnca_input_sensitivity(void* model, const float* x_nhwc, int batch, double* sums) {
    MODEL(model);
    if (!sums) { set_error("null sums"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    if (x_nhwc) DN_TRY(stage_inputs(M, batch, x_nhwc, nullptr, false));
    else if (M->last_batch != batch) { set_error("input sensitivity without x: the last forward had %d slices, not %d", M->last_batch, batch); return DNNCA_ESTATE; }
    DN_TRY(M->input_sensitivity(M->x_stage, batch));
    HIP_TRY(hipMemcpyAsync(sums, M->sens_sums, (size_t)batch * M->desc.in_channels * 8, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return M->flush_profile();
}

int dnnca_integrated_gradients(void* model, const float* x_nhwc, int batch, int steps, int baseline, double* signed_sums, double* abs_sums,
                               double* endpoints, float* map) {
    MODEL(model);
    if (!signed_sums || !abs_sums || !endpoints) { set_error("null sums or endpoints"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    if (steps < 1 || steps > Model::kAttrMaxSteps) { set_error("integrated gradients: steps %d outside [1, %d]", steps, Model::kAttrMaxSteps); return DNNCA_EINVAL; }
    if (baseline != 0 && baseline != 1) { set_error("integrated gradients: baseline %d is neither 0 (black) nor 1 (slice mean)", baseline); return DNNCA_EINVAL; }
    DN_TRY(M->sens_refusal("integrated gradients"));
    if (x_nhwc) DN_TRY(stage_inputs(M, batch, x_nhwc, nullptr, false));
    else if (M->last_batch != batch) { set_error("integrated gradients without x: the last forward had %d slices, not %d", M->last_batch, batch); return DNNCA_ESTATE; }
    DN_TRY(M->integrated_gradients(M->x_stage, batch, steps, baseline, map != nullptr));
    const int C = M->desc.in_channels;
    std::vector<double> h((size_t)batch * (2 * C + 2));
    HIP_TRY(hipMemcpyAsync(h.data(), M->attr_out, h.size() * 8, hipMemcpyDeviceToHost, M->stream));
    if (map) HIP_TRY(hipMemcpyAsync(map, M->attr_acc, (size_t)batch * M->desc.height * M->desc.width * C * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    for (int i = 0; i < batch * C; ++i) {
        signed_sums[i] = h[(size_t)2 * i];
        abs_sums[i] = h[(size_t)2 * i + 1];
    }
    const double* e = h.data() + (size_t)batch * C * 2;
    for (int b = 0; b < batch; ++b) {
        endpoints[2 * b] = e[b];                  // F(x)
        endpoints[2 * b + 1] = e[batch + b];      // F(x0)
    }
    return M->flush_profile();
}

int dnnca_last_step_out(void* model, dnnca_step_out* out) {
    MODEL(model);
    if (!out) return DNNCA_EINVAL;
    return read_out(M, M->world, out);
}

// ---- input pipeline: staging ring + copy stream (model.h) ------------------------------------------------------------------
static size_t stage_align(size_t b) { return (b + 255) & ~(size_t)255; }

int dnnca_stage_init(void* model, int slots, size_t bytes_per_slot) {
    MODEL(model);
    if (slots < 1 || slots > Model::kStageSlots) { set_error("staging slots %d outside [1, %d]", slots, Model::kStageSlots); return DNNCA_EINVAL; }
    if (M->stage_slots) { set_error("the staging ring exists already"); return DNNCA_ESTATE; }
    const size_t xb = (size_t)M->desc.max_batch * M->desc.height * M->desc.width * M->desc.in_channels * 4;
    const size_t yb = (size_t)M->desc.max_batch * M->outH * M->outW * 4;
    if (bytes_per_slot < stage_align(xb) + yb) bytes_per_slot = stage_align(xb) + yb;      // at least one float batch (x, y)
    HIP_TRY(hipStreamCreateWithFlags(&M->copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipHostMalloc((void**)&M->out_ring, (size_t)Model::kStageSlots * 8 * sizeof(float), hipHostMallocDefault));
    for (int i = 0; i < slots; ++i) {
        Model::StageSlot& sl = M->stage[i];
        DN_TRY(M->alloc((void**)&sl.x, stage_align(bytes_per_slot)));
        HIP_TRY(hipEventCreateWithFlags(&sl.uploaded, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    M->stage_bytes = stage_align(bytes_per_slot);
    M->stage_slots = slots;
    HIP_TRY(hipStreamSynchronize(M->stream));          // the allocations' memsets: nothing of them is left for the copy stream to race
    return DNNCA_OK;
}

// May be called from other host threads (each working on slots of its own) while the owning thread enqueues steps: it touches
// only the slot it was handed, the copy stream and the HIP runtime.  With pageable host memory the call returns when the copy is done;
// the GPU keeps working on the main stream meanwhile.
int dnnca_stage_upload(void* model, int slot, const void* host_a, size_t bytes_a, const void* host_b, size_t bytes_b,
                       void** a_dev, void** b_dev) {
    MODEL(model);
    DN_TRY(check_slot(M, slot));
    if (stage_align(bytes_a) + bytes_b > M->stage_bytes) {
        set_error("staging slot holds %zu bytes, asked for %zu + %zu", M->stage_bytes, bytes_a, bytes_b);
        return DNNCA_EINVAL;
    }
    HIP_TRY(hipSetDevice(M->device));                  // the current device is per host thread
    Model::StageSlot& sl = M->stage[slot];
    char* base = reinterpret_cast<char*>(sl.x);
    if (sl.has_done) HIP_TRY(hipStreamWaitEvent(M->copy_stream, sl.done, 0));      // the step that read the slot's last batch
    if (host_a && bytes_a) HIP_TRY(hipMemcpyAsync(base, host_a, bytes_a, hipMemcpyHostToDevice, M->copy_stream));
    if (host_b && bytes_b) HIP_TRY(hipMemcpyAsync(base + stage_align(bytes_a), host_b, bytes_b, hipMemcpyHostToDevice, M->copy_stream));
    HIP_TRY(hipEventRecord(sl.uploaded, M->copy_stream));
    if (a_dev) *a_dev = base;
    if (b_dev) *b_dev = base + stage_align(bytes_a);
    return DNNCA_OK;
}

int dnnca_stage_uploaded(void* model, int slot) {
    MODEL(model);
    DN_TRY(check_slot(M, slot));
    HIP_TRY(hipEventSynchronize(M->stage[slot].uploaded));
    return DNNCA_OK;
}

int dnnca_stage_wait(void* model, int slot) {
    MODEL(model);
    DN_TRY(check_slot(M, slot));
    HIP_TRY(hipStreamWaitEvent(M->stream, M->stage[slot].uploaded, 0));
    return DNNCA_OK;
}

// a staged step: the main stream waits for the slot's upload ...
static int staged_begin(Model* M, int slot, int batch) {
    DN_TRY(check_slot(M, slot));
    DN_TRY(check_batch(M, batch));
    HIP_TRY(hipStreamWaitEvent(M->stream, M->stage[slot].uploaded, 0));
    return DNNCA_OK;
}

// ... and sends its outputs to the slot's row of the pinned ring, `done` behind them
static int staged_end(Model* M, int slot, int batch, bool is_eval) {
    Model::StageSlot& sl = M->stage[slot];
    HIP_TRY(hipMemcpyAsync(M->out_ring + slot * 8, M->out5, 5 * sizeof(float), hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipEventRecord(sl.done, M->stream));
    sl.has_done = true;
    sl.is_eval = is_eval;
    sl.batch = batch;
    return DNNCA_OK;
}

int dnnca_train_step_staged(void* model, int slot, const float* x_dev, const float* y_dev, int batch, float lr,
                            const dnnca_loss_cfg* cfg) {
    MODEL(model);
    DN_TRY(M->ema_refuse("dnnca_train_step_staged"));
    DN_TRY(staged_begin(M, slot, batch));
    DN_TRY(train_step_impl(M, x_dev, y_dev, batch, lr, cfg, nullptr, slot));
    return staged_end(M, slot, batch, false);
}

int dnnca_staged_out(void* model, int slot, dnnca_step_out* out) {
    MODEL(model);
    if (!out) return DNNCA_EINVAL;
    if (slot < 0 || slot >= M->stage_slots || !M->stage[slot].has_done) { set_error("staging slot %d has run no step", slot); return DNNCA_ESTATE; }
    HIP_TRY(hipEventSynchronize(M->stage[slot].done));
    if (M->prof_mode) DN_TRY(M->flush_profile());
    // evaluation is rank-local: the loss slot was not all-reduced
    return convert_out(M->out_ring + slot * 8, M->stage[slot].is_eval ? 1 : M->world, out);
}

// ---- staged evaluation: keras Model.evaluate (engine.py:198-203) over the staging ring ---------------------------------
int dnnca_eval_begin(void* model, const float* thresholds, int n) {
    MODEL(model);
    DN_TRY(check_thresholds(thresholds, n));
    if (!M->stage_slots) { set_error("dnnca_eval_begin before dnnca_stage_init"); return DNNCA_ESTATE; }
    M->eval_thr.n = 0;
    if (n > 0) DN_TRY(confusion_begin(M, thresholds, n));
    M->eval_active = true;
    M->region_eval = false;
    return DNNCA_OK;
}

int dnnca_eval_step_staged(void* model, int slot, const float* x_dev, const float* y_dev, int batch, const dnnca_loss_cfg* cfg) {
    MODEL(model);
    if (!M->eval_active) { set_error("dnnca_eval_step_staged outside dnnca_eval_begin .. dnnca_eval_end"); return DNNCA_ESTATE; }
    if (!cfg) { set_error("null loss cfg"); return DNNCA_EINVAL; }
    DN_TRY(staged_begin(M, slot, batch));
    DN_TRY(M->forward(x_dev, batch, false));
    DN_TRY(M->loss_and_backward(y_dev, batch, *cfg, false));
    // the metrics see the labels as given (a smoothed copy exists only inside the loss, utils/losses.py:62-67)
    if (M->eval_thr.n > 0) confusion_add(M, (size_t)batch * M->outH * M->outW, y_dev);
    if (M->region_eval) DN_TRY(region_accumulate(M, M->prob, y_dev, batch, M->outH, M->outW));
    return staged_end(M, slot, batch, true);
}

int dnnca_eval_end(void* model, dnnca_confusion* out) {
    MODEL(model);
    if (!M->eval_active) { set_error("dnnca_eval_end without dnnca_eval_begin"); return DNNCA_ESTATE; }
    M->eval_active = false;
    if (M->eval_thr.n > 0 && !out) { set_error("null confusion output"); return DNNCA_EINVAL; }
    if (M->eval_thr.n > 0) return confusion_finish(M, out);
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

// ---- per-step training metrics (dnnca_train_metrics) ---------------------------------------------------------------------
int dnnca_train_metrics(void* model, const float* thresholds, int n) {
    MODEL(model);
    DN_TRY(check_thresholds(thresholds, n));
    HIP_TRY(hipStreamSynchronize(M->stream));          // steps in flight keep the thresholds they were enqueued with
    for (int& r : M->tm_ran) r = 0;
    M->tm_thr.n = 0;
    if (n == 0) return DNNCA_OK;
    if (!M->tm_thr.dev) {
        DN_TRY(M->alloc((void**)&M->tm_thr.dev, DNNCA_CONF_MAX_THR * 4));
        DN_TRY(M->alloc((void**)&M->tm_scratch, (Model::kTmRow + 1) * 8));
        DN_TRY(M->alloc((void**)&M->tm_hist, (size_t)(Model::kStageSlots + 1) * Model::kTmRow * 8));
        HIP_TRY(hipHostMalloc((void**)&M->tm_pin, (size_t)(Model::kStageSlots + 1) * Model::kTmRow * 8, hipHostMallocDefault));
    }
    return conf_thresholds_set(M, M->tm_thr, thresholds, n);
}

static int train_metrics_read(Model* M, int row, dnnca_confusion* out) {
    if (!out) { set_error("null confusion output"); return DNNCA_EINVAL; }
    const int n = M->tm_ran[row];
    if (n == 0 || n != M->tm_thr.n) { set_error("the step has no training-metric counts (dnnca_train_metrics off when it ran)"); return DNNCA_ESTATE; }
    confusion_from_hist(M->tm_pin + (size_t)row * Model::kTmRow, M->tm_thr, out);
    return DNNCA_OK;
}

int dnnca_last_step_confusion(void* model, dnnca_confusion* out) {
    MODEL(model);
    HIP_TRY(hipStreamSynchronize(M->stream));
    return train_metrics_read(M, Model::kStageSlots, out);
}

int dnnca_staged_confusion(void* model, int slot, dnnca_confusion* out) {
    MODEL(model);
    if (slot < 0 || slot >= M->stage_slots || !M->stage[slot].has_done || M->stage[slot].is_eval) {
        set_error("staging slot %d has run no train step", slot);
        return DNNCA_ESTATE;
    }
    HIP_TRY(hipEventSynchronize(M->stage[slot].done));
    return train_metrics_read(M, slot, out);
}

int dnnca_get_prob(void* model, float* prob_out, int64_t n_pixels) {
    MODEL(model);
    if (!prob_out || n_pixels < 0 || n_pixels > (int64_t)M->desc.max_batch * M->outH * M->outW) { set_error("bad probability read"); return DNNCA_EINVAL; }
    HIP_TRY(hipMemcpyAsync(prob_out, M->prob, (size_t)n_pixels * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

// ---- region (Tversky) term of the loss (kernels_region_loss.hip) ---------------------------------------------------------
int dnnca_model_set_region_loss(void* model, const dnnca_region_loss* cfg) {
    MODEL(model);
    if (cfg) {
        if (const char* why = region_loss_invalid(*cfg)) { set_error("region loss: %s", why); return DNNCA_EINVAL; }
        // left out for want of a reference: the bf16-emulating oracle has no statement of this loss to test a bf16 step against
        if (M->desc.dtype != DNNCA_F32) { set_error("region loss needs a dtype f32 model (this one is bf16)"); return DNNCA_EINVAL; }
        if (M->topk.fraction > 0.0 && !(cfg->crossentropy_weight > 0.f)) {
            set_error("region loss: crossentropy_weight must be > 0 while the top-k cross-entropy is on (dnnca_model_set_topk_loss)");
            return DNNCA_EINVAL;
        }
    }
    HIP_TRY(hipStreamSynchronize(M->stream));          // steps in flight keep the loss they were enqueued with
    M->region_loss.on = false;
    M->region_loss.sums_batch = 0;
    M->boundary.sums_batch = 0;
    if (!cfg) {                                         // the boundary term rides the region loss's launches: it goes with them
        M->boundary.weight = 0.f;
        M->boundary.batch = 0;
        M->topk.fraction = 0.0;                         // ... and so does the top-k cross-entropy
        M->topk.batch = 0;
        return DNNCA_OK;
    }
    DN_TRY(region_loss_prepare(M));
    M->region_loss.cfg = *cfg;
    M->region_loss.on = true;
    return DNNCA_OK;
}

int dnnca_region_loss_sums(void* model, int batch, double* out) {
    MODEL(model);
    if (!out) { set_error("null region-loss sums"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    if (!M->region_loss.ws || M->region_loss.sums_batch < batch) {
        set_error("no step with the region loss has run on %d images (dnnca_model_set_region_loss)", batch);
        return DNNCA_ESTATE;
    }
    std::vector<double> st((size_t)batch * kRlStat);
    HIP_TRY(hipMemcpyAsync(st.data(), M->region_loss.ws, st.size() * 8, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    for (int b = 0; b < batch; ++b)
        for (int k = 0; k < 3; ++k) out[b * 3 + k] = st[(size_t)b * kRlStat + k];
    return DNNCA_OK;
}

// ---- boundary (signed-distance) term of the loss (kernels_boundary.hip, kernels_region_loss.hip) ----------------------------
int dnnca_model_set_boundary_loss(void* model, float boundary_weight) {
    MODEL(model);
    if (!(std::isfinite(boundary_weight) && boundary_weight >= 0.f)) { set_error("boundary loss: boundary_weight must be >= 0 and finite"); return DNNCA_EINVAL; }
    if (!M->region_loss.on) {
        set_error("boundary loss: no region loss is set (dnnca_model_set_region_loss): the term rides its launches");
        return DNNCA_EINVAL;
    }
    if (M->outH > kSurfaceMaxSide || M->outW > kSurfaceMaxSide) {
        set_error("boundary loss: labels of %d x %d exceed %d pixels a side", M->outH, M->outW, kSurfaceMaxSide);
        return DNNCA_EINVAL;
    }
    HIP_TRY(hipStreamSynchronize(M->stream));          // steps in flight keep the loss they were enqueued with
    if (boundary_weight > 0.f && !M->boundary.phi) {
        const size_t n = (size_t)M->desc.max_batch * M->outH * M->outW;
        DN_TRY(M->alloc((void**)&M->boundary.cols, n * 4));
        DN_TRY(M->alloc((void**)&M->boundary.phi, n * 4));
    }
    M->boundary.weight = boundary_weight;
    M->boundary.batch = M->boundary.sums_batch = 0;
    return DNNCA_OK;
}

int dnnca_boundary_loss_sums(void* model, int batch, double* out) {
    MODEL(model);
    if (!out) { set_error("null boundary-loss sums"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    if (!M->region_loss.ws || M->boundary.sums_batch < batch) {
        set_error("no step with the boundary loss has run on %d images (dnnca_model_set_boundary_loss)", batch);
        return DNNCA_ESTATE;
    }
    std::vector<double> st((size_t)batch * kRlStat);
    HIP_TRY(hipMemcpyAsync(st.data(), M->region_loss.ws, st.size() * 8, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    for (int b = 0; b < batch; ++b) out[b] = st[(size_t)b * kRlStat + 7];
    return DNNCA_OK;
}

int dnnca_boundary_distance(void* model, int batch, float* phi_out) {
    MODEL(model);
    if (!phi_out) { set_error("null boundary distance map"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    if (!M->boundary.phi || M->boundary.batch < batch) {
        set_error("no step with the boundary loss has run on %d images (dnnca_model_set_boundary_loss)", batch);
        return DNNCA_ESTATE;
    }
    HIP_TRY(hipMemcpyAsync(phi_out, M->boundary.phi, (size_t)batch * M->outH * M->outW * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

// ---- top-k (hard-pixel) cross-entropy (kernels_topk.hip, kernels_region_loss.hip) ------------------------------------------
int dnnca_model_set_topk_loss(void* model, double fraction) {
    MODEL(model);
    if (!(std::isfinite(fraction) && fraction >= 0.0 && fraction <= 1.0)) { set_error("top-k loss: the fraction must be in (0, 1], or 0 for off"); return DNNCA_EINVAL; }
    if (!M->region_loss.on) {
        set_error("top-k loss: no region loss is set (dnnca_model_set_region_loss): the term rides its launches");
        return DNNCA_EINVAL;
    }
    if (fraction > 0.0 && !(M->region_loss.cfg.crossentropy_weight > 0.f)) {
        set_error("top-k loss: the region loss's crossentropy_weight is 0: there is no cross-entropy to take the top k of");
        return DNNCA_EINVAL;
    }
    HIP_TRY(hipStreamSynchronize(M->stream));          // steps in flight keep the loss they were enqueued with
    if (fraction > 0.0 && !M->topk.plane) {
        DN_TRY(M->alloc((void**)&M->topk.ws, topk_ws_bytes(M->desc.max_batch)));          // (zeroed: the histograms start empty)
        DN_TRY(M->alloc((void**)&M->topk.plane, (size_t)M->desc.max_batch * M->outH * M->outW * 4));
    }
    M->topk.fraction = fraction;
    M->topk.batch = 0;
    return DNNCA_OK;
}

int dnnca_topk_loss_state(void* model, int batch, int32_t* k_out, int32_t* n_kept_out, float* tau_out, double* sum_out) {
    MODEL(model);
    if (!k_out || !n_kept_out || !tau_out || !sum_out) { set_error("null top-k loss state"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    if (!M->topk.ws || M->topk.batch < batch) {
        set_error("no step with the top-k loss has run on %d images (dnnca_model_set_topk_loss)", batch);
        return DNNCA_ESTATE;
    }
    std::vector<TopkImage> st((size_t)batch);
    HIP_TRY(hipMemcpyAsync(st.data(), M->topk.ws, st.size() * sizeof(TopkImage), hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    for (int b = 0; b < batch; ++b) {
        k_out[b] = (int32_t)st[b].k;
        n_kept_out[b] = (int32_t)st[b].n_kept;
        memcpy(tau_out + b, &st[b].tau, 4);
        sum_out[b] = st[b].sum;
    }
    return DNNCA_OK;
}

int dnnca_topk_pixel_loss(void* model, int batch, float* out) {
    MODEL(model);
    if (!out) { set_error("null top-k pixel loss"); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    if (!M->topk.plane || M->topk.batch < batch) {
        set_error("no step with the top-k loss has run on %d images (dnnca_model_set_topk_loss)", batch);
        return DNNCA_ESTATE;
    }
    HIP_TRY(hipMemcpyAsync(out, M->topk.plane, (size_t)batch * M->outH * M->outW * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

int dnnca_sync(void* model) {
    MODEL(model);
    HIP_TRY(hipStreamSynchronize(M->stream));
    return M->flush_profile();
}

int dnnca_dev_alloc(void** dev_ptr, size_t bytes) {
    if (!dev_ptr) return DNNCA_EINVAL;
    HIP_TRY(hipMalloc(dev_ptr, bytes ? bytes : 4));
    return DNNCA_OK;
}
int dnnca_dev_free(void* dev_ptr) { HIP_TRY(hipFree(dev_ptr)); return DNNCA_OK; }
int dnnca_memcpy_h2d(void* dev_dst, const void* host_src, size_t bytes) { HIP_TRY(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice)); return DNNCA_OK; }
int dnnca_memcpy_d2h(void* host_dst, const void* dev_src, size_t bytes) { HIP_TRY(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost)); return DNNCA_OK; }

// ------------------------------------------------------------------------------------------------- data parallel
int dnnca_comm_unique_id(void* id_out) {
    if (!id_out) return DNNCA_EINVAL;
    static_assert(sizeof(ncclUniqueId) <= DNNCA_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) { set_error("ncclGetUniqueId: %s", ncclGetErrorString(r)); return DNNCA_ECOMM; }
    memset(id_out, 0, DNNCA_UNIQUE_ID_BYTES);
    memcpy(id_out, &id, sizeof(id));
    return DNNCA_OK;
}

int dnnca_comm_init(void* model, int rank, int world, const void* unique_id, size_t id_len) {
    MODEL(model);
    if (world < 1 || rank < 0 || rank >= world) { set_error("bad rank/world %d/%d", rank, world); return DNNCA_EINVAL; }
    M->rank = rank;
    M->world = world;
    // DNNCA_FORCE_RCCL: build a one-rank communicator too, so every collective of the DP path can be exercised on one GPU
    if (world == 1 && !(M->sw.force_rccl && unique_id)) return DNNCA_OK;
    if (!unique_id || id_len < sizeof(ncclUniqueId)) { set_error("unique id too short"); return DNNCA_EINVAL; }
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    ncclResult_t r = ncclCommInitRank(&M->comm, world, id, rank);
    if (r != ncclSuccess) { set_error("ncclCommInitRank: %s", ncclGetErrorString(r)); M->comm = nullptr; M->world = 1; return DNNCA_ECOMM; }
    return DNNCA_OK;
}

int dnnca_comm_world(void* model, int* rank, int* world) {
    MODEL(model);
    if (rank) *rank = M->rank;
    if (world) *world = M->world;
    return DNNCA_OK;
}

int dnnca_comm_collectives(void* model, int* count) {
    MODEL(model);
    if (!count) return DNNCA_EINVAL;
    *count = M->collectives_last_step;
    return DNNCA_OK;
}

int dnnca_comm_collective_floats(void* model, int64_t* count) {
    MODEL(model);
    if (!count) return DNNCA_EINVAL;
    *count = M->collective_floats_last_step;
    return DNNCA_OK;
}

int dnnca_comm_broadcast_weights(void* model, int root) {
    MODEL(model);
    if (!M->comm) return DNNCA_OK;
    DN_TRY(M->ema_refuse("dnnca_comm_broadcast_weights"));
    // ... and the weight average with its update count, when it is on (on every rank or on none)
    struct { float* p; int64_t n; } bufs[5] = {{M->p, M->nT}, {M->state, M->nS}, {M->m, M->nT}, {M->v, M->nT}, {M->ema.e, M->ema.e ? M->nT : 0}};
    if (M->ema.e) {
        int64_t* cnt = reinterpret_cast<int64_t*>(M->conf_dev);
        HIP_TRY(hipMemcpyAsync(cnt, &M->ema.num_updates, 8, hipMemcpyHostToDevice, M->stream));
        ncclResult_t r = ncclBroadcast(cnt, cnt, 1, ncclInt64, root, M->comm, M->stream);
        if (r != ncclSuccess) { set_error("ncclBroadcast: %s", ncclGetErrorString(r)); return DNNCA_ECOMM; }
        HIP_TRY(hipMemcpyAsync(&M->ema.num_updates, cnt, 8, hipMemcpyDeviceToHost, M->stream));
        HIP_TRY(hipStreamSynchronize(M->stream));
    }
    for (auto& b : bufs) {
        if (b.n == 0) continue;
        ncclResult_t r = ncclBroadcast(b.p, b.p, (size_t)b.n, ncclFloat, root, M->comm, M->stream);
        if (r != ncclSuccess) { set_error("ncclBroadcast: %s", ncclGetErrorString(r)); return DNNCA_ECOMM; }
    }
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

int dnnca_comm_average_state(void* model) {
    MODEL(model);
    if (!M->comm || M->nS == 0) return DNNCA_OK;
    ncclResult_t r = ncclAllReduce(M->state, M->state, (size_t)M->nS, ncclFloat, ncclSum, M->comm, M->stream);
    if (r != ncclSuccess) { set_error("ncclAllReduce(state): %s", ncclGetErrorString(r)); return DNNCA_ECOMM; }
    g_scale(M->stream, (size_t)M->nS, M->state, 1.0f / (float)M->world);
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

int dnnca_comm_allreduce_host(void* model, double* values, int64_t n, int op) {
    MODEL(model);
    if (n < 1 || !values) { set_error("dnnca_comm_allreduce_host: bad arguments (n = %lld)", (long long)n); return DNNCA_EINVAL; }
    if (op != 0 && op != 1) { set_error("dnnca_comm_allreduce_host: op %d (0 sum, 1 max)", op); return DNNCA_EINVAL; }
    if (!M->comm) return DNNCA_OK;
    // doubles: pixel counts of a whole validation set stay exact (float32 stops at 2^24 = 64 slices of 512 x 512);
    // chunked through the confusion staging buffer, so any length works
    double* tmp = reinterpret_cast<double*>(M->conf_dev);
    const int64_t cap = 2 * (DNNCA_CONF_MAX_THR + 1);
    for (int64_t off = 0; off < n; off += cap) {
        size_t c = (size_t)std::min<int64_t>(cap, n - off);
        HIP_TRY(hipMemcpyAsync(tmp, values + off, c * 8, hipMemcpyHostToDevice, M->stream));
        ncclResult_t r = ncclAllReduce(tmp, tmp, c, ncclDouble, op == 1 ? ncclMax : ncclSum, M->comm, M->stream);
        if (r != ncclSuccess) { set_error("ncclAllReduce(host): %s", ncclGetErrorString(r)); return DNNCA_ECOMM; }
        HIP_TRY(hipMemcpyAsync(values + off, tmp, c * 8, hipMemcpyDeviceToHost, M->stream));
        HIP_TRY(hipStreamSynchronize(M->stream));
    }
    return DNNCA_OK;
}

// ------------------------------------------------------------------------------------------------- measurement
int dnnca_timer_start(void* model) {
    MODEL(model);
    HIP_TRY(hipEventRecord(M->ev0, M->stream));
    return DNNCA_OK;
}

int dnnca_timer_stop(void* model, float* elapsed_ms) {
    MODEL(model);
    HIP_TRY(hipEventRecord(M->ev1, M->stream));
    HIP_TRY(hipEventSynchronize(M->ev1));
    if (elapsed_ms) HIP_TRY(hipEventElapsedTime(elapsed_ms, M->ev0, M->ev1));
    return M->flush_profile();
}

int dnnca_profile_enable(void* model, int mode) {
    MODEL(model);
    DN_TRY(M->flush_profile());
    M->prof_mode = mode;
    return DNNCA_OK;
}

int dnnca_profile_focus(void* model, const char* kernel_name) {
    MODEL(model);
    M->focus = kernel_name ? kernel_name : "";
    return DNNCA_OK;
}

int dnnca_profile_sample(void* model, int period) {
    MODEL(model);
    if (period < 1) { set_error("period must be >= 1"); return DNNCA_EINVAL; }
    M->prof_period = period;
    return DNNCA_OK;
}

int dnnca_profile_reset(void* model) {
    MODEL(model);
    DN_TRY(M->flush_profile());
    M->kstats.clear();
    M->kid.clear();
    return DNNCA_OK;
}

int dnnca_profile_count(void* model, int* count) {
    MODEL(model);
    DN_TRY(M->flush_profile());
    *count = (int)M->kstats.size();
    return DNNCA_OK;
}

int dnnca_profile_get(void* model, int index, char* name, size_t name_cap, int64_t* launches, double* total_ms,
                      double* algorithmic_bytes, double* flops) {
    MODEL(model);
    if (index < 0 || index >= (int)M->kstats.size()) { set_error("profile index out of range"); return DNNCA_EINVAL; }
    const KStat& k = M->kstats[index];
    if (name && name_cap) snprintf(name, name_cap, "%s", k.name.c_str());
    if (launches) *launches = k.launches;
    if (total_ms) *total_ms = k.total_ms;
    double L = k.launches ? (double)k.launches : 1.0;
    if (algorithmic_bytes) *algorithmic_bytes = k.bytes / L;
    if (flops) *flops = k.flops / L;
    return DNNCA_OK;
}

// development aid (not part of include/dnnca.h): copy the first `n` 64-bit stamps of the tuned backward kernel
int dnnca_debug_read_stamps(void* model, unsigned long long* out, int n) {
    MODEL(model);
    unsigned long long* s = fast_debug_stamps(M);
    if (!s) { set_error("no stamps"); return DNNCA_ESTATE; }
    HIP_TRY(hipStreamSynchronize(M->stream));
    HIP_TRY(hipMemcpy(out, s, (size_t)n * 8, hipMemcpyDeviceToHost));
    return DNNCA_OK;
}

// development aid (not part of include/dnnca.h): n back-to-back launches of a trivial kernel on the model's stream
__global__ void k_noop(float* p) { if (p == nullptr) *p = 0.f; }
int dnnca_debug_launch_cost(void* model, int n, int blocks, float* us_per_launch) {
    MODEL(model);
    HIP_TRY(hipStreamSynchronize(M->stream));
    HIP_TRY(hipEventRecord(M->ev0, M->stream));
    for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_noop, dim3(blocks), dim3(256), 0, M->stream, M->prob);
    HIP_TRY(hipEventRecord(M->ev1, M->stream));
    HIP_TRY(hipEventSynchronize(M->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, M->ev0, M->ev1));
    *us_per_launch = ms * 1000.f / n;
    return DNNCA_OK;
}

// pass DNNCA_PLAN_TRAIN: forward(training) + backward + optimizer, exactly what dnnca_train_step enqueues; DNNCA_PLAN_EVAL: what
// dnnca_eval_step / dnnca_eval_step_staged enqueue (without the metric accumulation the caller switches on); DNNCA_PLAN_FORWARD:
// dnnca_forward / dnnca_forward_dev with training = 0.  Nothing is launched and no variable, state or later result changes (the one-time plan
// tables of the first forward pass may be built by it).
int dnnca_plan_dump_pass(void* model, int pass, int batch, char* buf, size_t cap) {
    MODEL(model);
    if (!buf || !cap) return DNNCA_EINVAL;
    if (pass != DNNCA_PLAN_TRAIN && pass != DNNCA_PLAN_EVAL && pass != DNNCA_PLAN_FORWARD && pass != DNNCA_PLAN_SENSITIVITY &&
        pass != DNNCA_PLAN_LESION && pass != DNNCA_PLAN_LESION_LINKED && pass != DNNCA_PLAN_LESION_MATCHED &&
        pass != DNNCA_PLAN_SURFACE && pass != DNNCA_PLAN_ATTRIBUTION && pass != DNNCA_PLAN_LESION_FEATURES &&
        pass != DNNCA_PLAN_DETECTION) { set_error("unknown plan pass %d", pass); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    M->plan_text.clear();
    M->dry = true;
    dnnca_loss_cfg cfg = {0, 0.f, 0.f, 1.f};
    const int B = batch;
    int rc;
    if (pass == DNNCA_PLAN_TRAIN) {
        rc = train_pass(M, M->x_stage, M->y_stage, B, 1e-3f, cfg, Model::kStageSlots);
    } else if (pass == DNNCA_PLAN_EVAL) {
        rc = M->forward(M->x_stage, B, false);
        if (rc == DNNCA_OK) rc = M->loss_and_backward(M->y_stage, B, cfg, false);
    } else if (pass == DNNCA_PLAN_SENSITIVITY) {
        rc = M->input_sensitivity(M->x_stage, B);
    } else if (pass == DNNCA_PLAN_ATTRIBUTION) {
        rc = M->integrated_gradients(M->x_stage, B, M->attr_steps_last, M->attr_baseline_last, true);
    } else if (pass == DNNCA_PLAN_LESION || pass == DNNCA_PLAN_LESION_LINKED) {
        LesionArgs a;
        bool want_mask = true;
        lesion_last(M, &a.rf, &a.k, &want_mask);
        rc = lesion_check(a, M->outH, M->outW);
        if (rc == DNNCA_OK && pass == DNNCA_PLAN_LESION)
            rc = lesion_table(M, M->prob, B, M->outH, M->outW, a, nullptr, nullptr, nullptr, nullptr, want_mask);
        else if (rc == DNNCA_OK)
            rc = lesion_table_linked(M, M->prob, B, M->outH, M->outW, a, nullptr, nullptr, nullptr, nullptr, want_mask, nullptr, nullptr,
                                     nullptr);
    } else if (pass == DNNCA_PLAN_LESION_MATCHED) {
        LesionArgs a;
        bool want_mask = true;
        lesion_match_last(M, &a.rf, &a.k, &want_mask);
        rc = lesion_check(a, M->outH, M->outW);
        if (rc == DNNCA_OK)
            rc = lesion_table_matched(M, M->prob, M->y_stage, B, M->outH, M->outW, a, nullptr, nullptr, nullptr, want_mask, nullptr, nullptr);
    } else if (pass == DNNCA_PLAN_LESION_FEATURES) {
        LesionArgs a;
        bool want_mask = true;
        int bins = 32, ring = 3;
        lesion_features_last(M, &a.rf, &a.k, &want_mask, &bins, &ring);
        rc = lesion_check(a, M->outH, M->outW);
        if (rc == DNNCA_OK) rc = lesion_features_check(a, M->desc.in_channels, bins, ring);
        if (rc == DNNCA_OK)
            rc = lesion_table_features(M, M->prob, M->x_stage, M->desc.in_channels, B, M->outH, M->outW, a, nullptr, nullptr, nullptr,
                                       nullptr, want_mask, bins, ring, nullptr, nullptr, nullptr, nullptr);
    } else if (pass == DNNCA_PLAN_SURFACE) {
        LesionArgs a;
        surface_last(M, &a.rf, &a.k);
        rc = lesion_check(a, M->outH, M->outW);
        if (rc == DNNCA_OK)
            rc = surface_distances(M, M->prob, M->y_stage, B, M->outH, M->outW, a, 1, nullptr, nullptr, nullptr, nullptr);
    } else if (pass == DNNCA_PLAN_DETECTION) {
        rc = detection_map(M, M->prob, M->prob, B, M->outH, M->outW, M->detect_last, nullptr, nullptr, nullptr, nullptr);
    } else {
        rc = dnnca_forward_dev(model, M->x_stage, B, 0);
    }
    M->dry = false;
    snprintf(buf, cap, "%s", M->plan_text.c_str());
    return rc;
}

int dnnca_plan_dump(void* model, char* buf, size_t cap) {
    MODEL(model);
    return dnnca_plan_dump_pass(model, DNNCA_PLAN_TRAIN, M->desc.max_batch, buf, cap);
}

}  // extern "C"
