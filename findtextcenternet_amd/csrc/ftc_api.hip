// C ABI (include/ftc.h): plan validation / execution and the decode entry point.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "ftc_common.h"
#include "ftc_host.h"

hipError_t launch_decode(const float* heat, const float* feat, int B, int h, int w, int C, const ftc_tile* tiles,
                         float logit_cut, int scale, int max_boxes, float* boxes, int box_stride, float* feats, int feat_stride,
                         int32_t* index, int32_t* counts, void* scratch, hipStream_t s);

hipError_t launch_tile_gather(const unsigned char* page, int PH, int PW, const int* origins, int B, int th, int tw, float* out,
                              hipStream_t s);
hipError_t launch_adamw_sf(const ftc_mt_chunk* chunks, int n_chunks, float beta2, float one_minus_beta2, float bias_correction2, float eps,
                           float decay, float ckp1, float y_alpha, float lr, int write_grad, hipStream_t s);
hipError_t launch_box_hists(const float* loc, int N, const float* page, int PH, int PW, float cut_off, double* out, hipStream_t s);
hipError_t launch_greedy(const float* loc, const int* order, int N, const double* hist1, const double* th, float cut_off, double* kept,
                         int* keep_idx, int* hdr, double* rb, int* status, int* cnt, int* cursor, int* nbr, long edge_cap, unsigned int* fill_big,
                         long fill_big_words, int force_seq, const float* seps, const float* codes, int mh, int mw, int scale, float* out_loc,
                         int* out_idx, int* out_n, int variant, int seed_start, double seed_scale, float* out_cmax, hipStream_t s);
hipError_t launch_page_order(const float* loc, int N, const double* hist0, float cut_off, int* order, double* th, void* scratch, hipStream_t s);
hipError_t launch_paste_maps(const float* heat, const ftc_tile* tiles, int B, int h, int w, int scale, float* canv, int ph, int pw,
                             hipStream_t s);

hipError_t launch_topk_mask(const float* vals, long n, long k, unsigned char* mask, int32_t* sel_index, int32_t* count, hipStream_t s);
hipError_t launch_mask_compact(const unsigned char* mask, long n, int32_t* sel_index, long cap, int32_t* count, hipStream_t s);
hipError_t launch_gather_rows(const float* feat, const int32_t* sel_index, const int32_t* count, long cap, int C, int Cpad, void* rows, int out_dtype,
                              hipStream_t s);
hipError_t launch_losses(const float* heat, const long* hstrides, const float* label, const int32_t* idmap, int B, int h, int w, const float* const* dec,
                         const int* mod, const int32_t* sel_index, const int32_t* count, long cap, float* out, void* scratch, hipStream_t s);
hipError_t launch_cov_step(const float* L, int n, int iter, float* state, float* out_loss, hipStream_t s);

// Per-device launch state shared by the launchers (ftc_host.h).  One lock for both: taken for a set / vector lookup per launch, never contended
// in a single-threaded host loop; a first launch makes its HIP call under it, so a racing thread launches only after the attribute is set.
namespace {
std::mutex g_dev_mu;
std::set<std::pair<const void*, int>> g_lds_allowed;      // (kernel, device ordinal)
std::vector<int> g_dev_cus;                                // [device ordinal], 0 = not asked yet
}  // namespace

hipError_t ftc_allow_dyn_lds(const void* kernel, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_dev_mu);
    if (g_lds_allowed.count({kernel, dev})) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) g_lds_allowed.insert({kernel, dev});
    return e;
}

hipError_t ftc_device_cus(int* n_cu) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_dev_mu);
    if (dev >= (int)g_dev_cus.size()) g_dev_cus.resize(dev + 1, 0);
    if (g_dev_cus[dev] == 0 && (e = hipDeviceGetAttribute(&g_dev_cus[dev], hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    *n_cu = g_dev_cus[dev];
    return hipSuccess;
}

namespace {
// FTC_OP_LOSSES: ftc_losses on the NHWC [B,H,W,9] map block of the training plan
hipError_t launch_losses_op(const OpArgs& a, hipStream_t s) {
    const ftc_op& o = *a.op;
    const long hs[4] = {(long)o.H * o.W * 9, 1, (long)o.W * 9, 9};
    static const int mod[3] = {1091, 1093, 1097};                   // util_func.py:5 modulo_list
    const float* dec[3] = {(const float*)a.w2, a.bias, a.bias2};
    const bool has_dec = a.w2 && a.bias && a.bias2 && o.aux0 > 0;
    return launch_losses((const float*)a.in, hs, (const float*)a.in2, (const int32_t*)a.w, o.B, o.H, o.W, has_dec ? dec : nullptr, mod,
                         (const int32_t*)a.scale, nullptr, (long)o.aux0, (float*)a.out, a.aux, s);
}
}  // namespace

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int fail_hip(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return FTC_ERR_HIP;
}

// `extent` = bytes the op reads / writes from the operand's start (0 = unknown: only the start is checked).  The input / heat-map /
// feature bases are caller buffers whose sizes the plan does not know (ftc_forward derives them from B, H, W).
bool ref_ok(const ftc_ref& r, const ftc_plan* pl, bool required, int64_t extent, std::string* why) {
    if (r.base == FTC_BASE_NULL) {
        if (required) { *why = "missing required operand"; return false; }
        return true;
    }
    if (r.base < 0 || r.base >= FTC_NUM_BASES) { *why = "bad base id"; return false; }
    if (r.offset < 0 || (r.offset & 15)) { *why = "operand offset must be >= 0 and 16-byte aligned"; return false; }
    if (extent < 0) { *why = "operand size overflows"; return false; }
    const int64_t end = r.offset + (extent > 0 ? extent : 1);
    if (r.base == FTC_BASE_WORKSPACE && end > pl->workspace_bytes) { *why = "workspace operand out of range (offset + extent > workspace_bytes)"; return false; }
    if (r.base == FTC_BASE_WEIGHTS && end > pl->weights_bytes) { *why = "weights operand out of range (offset + extent > weights_bytes)"; return false; }
    return true;
}

// The op's form and the state and extent of each operand come from op_extents (op_extents.h); here every used operand is held to its base.
const char* validate_op(const ftc_op& o, const ftc_plan* pl, std::string* why) {
    OpExtents e;
    if (const char* refused = op_extents(o, &e)) return refused;
    for (int i = 0; i < FTC_NUM_OPERANDS; ++i) {
        std::string w;
        if (e.state[i] == FTC_OPERAND_UNUSED || ref_ok(op_operand(o, i), pl, e.state[i] == FTC_OPERAND_REQUIRED, e.bytes[i], &w)) continue;
        // (the one operand that is refused under the op's name, as it always was)
        if (o.kind == FTC_OP_LOSS_BWD && i == OPD_OUT2) return "loss_bwd: out2 / aux1 (padded logit row >= 1097, % 4 == 0)";
        *why = std::string(kOperandName[i]) + ": " + w;
        return why->c_str();
    }
    return nullptr;
}

inline void* resolve(const ftc_ref& r, void* const bases[FTC_NUM_BASES]) {
    if (r.base == FTC_BASE_NULL) return nullptr;
    return static_cast<char*>(bases[r.base]) + r.offset;
}

hipError_t run_one(const ftc_op& o, void* const bases[FTC_NUM_BASES], hipStream_t s) {
    OpArgs a;
    a.op = &o;
    a.in = resolve(o.in, bases);
    a.in2 = resolve(o.in2, bases);
    a.out = resolve(o.out, bases);
    a.w = resolve(o.w, bases);
    a.w2 = resolve(o.w2, bases);
    a.bias = static_cast<const float*>(resolve(o.bias, bases));
    a.bias2 = static_cast<const float*>(resolve(o.bias2, bases));
    a.scale = static_cast<const float*>(resolve(o.scale, bases));
    a.shift = static_cast<const float*>(resolve(o.shift, bases));
    a.aux = static_cast<float*>(resolve(o.aux, bases));
    a.out2 = resolve(o.out2, bases);
    switch (o.kind) {
    case FTC_OP_STEM: return launch_stem(a, s);
    case FTC_OP_CONV: return launch_conv(a, s);
    case FTC_OP_DWCONV: return launch_dwconv(a, s);
    case FTC_OP_SE: return launch_se(a, s);
    case FTC_OP_MBHEAD: return launch_mbhead(a, s);
    case FTC_OP_FMBCONV: return launch_fmbconv(a, s);
    case FTC_OP_UPCAT: return launch_upcat(a, s);
    case FTC_OP_NMS: return launch_nms(a, s);
    case FTC_OP_TAPSUM: return launch_tapsum(a, s);
    case FTC_OP_BNSTAT: return launch_bnstat(a, s);
    case FTC_OP_BNACT: return launch_bnact(a, s);
    case FTC_OP_GATHER_ROWS: return launch_gather_rows_op(a, s);
    case FTC_OP_LOSSES: return launch_losses_op(a, s);
    case FTC_OP_LOSS_BWD: return launch_loss_bwd(a, s);
    case FTC_OP_SCATTER_ROWS: return launch_scatter_rows(a, s);
    case FTC_OP_BNBWD: return launch_bnbwd(a, s);
    case FTC_OP_WGRAD: return launch_wgrad(a, s);
    case FTC_OP_DWBWD: return launch_dwbwd(a, s);
    case FTC_OP_SEBWD: return launch_sebwd(a, s);
    case FTC_OP_UPCATBWD: return launch_upcatbwd(a, s);
    case FTC_OP_DILATE: return launch_dilate(a, s);
    case FTC_OP_TOPDGRAD: return launch_topdgrad(a, s);
    case FTC_OP_COLSUM: return launch_colsum(a, s);
    case FTC_OP_STEMWGRAD: return launch_stemwgrad(a, s);
    case FTC_OP_FILL: return launch_fill(a, s);
    case FTC_OP_JOIN: return hipSuccess;
    default: return hipErrorInvalidValue;
    }
}

int check_bases(const ftc_plan* plan, void* const bases[FTC_NUM_BASES], int first, int last) {
    for (int i = first; i <= last; ++i) {
        const ftc_op& o = plan->ops[i];
        const ftc_ref* refs[] = {&o.in, &o.in2, &o.out, &o.w, &o.w2, &o.bias, &o.bias2, &o.scale, &o.shift, &o.aux, &o.out2};
        for (const ftc_ref* r : refs)
            if (r->base != FTC_BASE_NULL && bases[r->base] == nullptr)
                return fail(FTC_ERR_INVALID, "ftc_plan_run: op " + std::to_string(i) + " needs base " + std::to_string(r->base) + " which is NULL");
    }
    return FTC_OK;
}

}  // namespace

int ftc_set_error(int code, const std::string& msg) { return fail(code, msg); }

extern "C" {

int ftc_abi_version(void) { return FTC_ABI_VERSION; }

const char* ftc_last_error(void) { return g_err.c_str(); }

int ftc_device_info(int* n_cu, char* name, int name_len) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail(FTC_ERR_NO_DEVICE, std::string("hipGetDevice: ") + hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return fail(FTC_ERR_NO_DEVICE, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (name && name_len > 0) { std::strncpy(name, prop.gcnArchName, name_len - 1); name[name_len - 1] = 0; }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(FTC_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    return FTC_OK;
}

int ftc_plan_create(const ftc_op* ops, int n_ops, int64_t workspace_bytes, int64_t weights_bytes, ftc_plan** out) {
    if (!ops || n_ops <= 0 || !out) return fail(FTC_ERR_INVALID, "ftc_plan_create: null/empty arguments");
    ftc_plan* pl = new (std::nothrow) ftc_plan();
    if (!pl) return fail(FTC_ERR_NOMEM, "ftc_plan_create: out of host memory");
    pl->workspace_bytes = workspace_bytes;
    pl->weights_bytes = weights_bytes;
    pl->ops.assign(ops, ops + n_ops);
    for (int i = 0; i < n_ops; ++i) {
        std::string why;
        const char* bad = validate_op(pl->ops[i], pl, &why);
        if (bad) {
            std::string msg = "ftc_plan_create: op " + std::to_string(i) + " (kind " + std::to_string(pl->ops[i].kind) + "): " + bad;
            delete pl;
            return fail(FTC_ERR_INVALID, msg);
        }
    }
    *out = pl;
    return FTC_OK;
}

void ftc_plan_destroy(ftc_plan* plan) { delete plan; }

int ftc_plan_num_ops(const ftc_plan* plan) { return plan ? (int)plan->ops.size() : 0; }

int ftc_plan_run(const ftc_plan* plan, void* const bases[FTC_NUM_BASES], void* stream, int first_op, int last_op) {
    if (!plan || !bases) return fail(FTC_ERR_INVALID, "ftc_plan_run: null arguments");
    const int n = (int)plan->ops.size();
    if (last_op < 0 || last_op >= n) last_op = n - 1;
    if (first_op < 0) first_op = 0;
    if (first_op > last_op) return fail(FTC_ERR_INVALID, "ftc_plan_run: empty op range");
    int rc = check_bases(plan, bases, first_op, last_op);
    if (rc != FTC_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int i = first_op; i <= last_op; ++i) {
        hipError_t e = run_one(plan->ops[i], bases, s);
        if (e != hipSuccess) {
            char buf[64];
            std::snprintf(buf, sizeof buf, "ftc_plan_run: op %d (kind %d)", i, plan->ops[i].kind);
            return fail_hip(e, buf);
        }
    }
    return FTC_OK;
}

int ftc_plan_run_streams(const ftc_plan* plan, void* const bases[FTC_NUM_BASES], void* stream, void* side_stream, int first_op, int last_op) {
    if (!side_stream) return ftc_plan_run(plan, bases, stream, first_op, last_op);
    if (!plan || !bases) return fail(FTC_ERR_INVALID, "ftc_plan_run_streams: null arguments");
    const int n = (int)plan->ops.size();
    if (last_op < 0 || last_op >= n) last_op = n - 1;
    if (first_op < 0) first_op = 0;
    if (first_op > last_op) return fail(FTC_ERR_INVALID, "ftc_plan_run_streams: empty op range");
    int rc = check_bases(plan, bases, first_op, last_op);
    if (rc != FTC_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream), s2 = static_cast<hipStream_t>(side_stream);
    // the two events belong to this call (a plan may be run from several host threads); destroying an event with work pending is legal
    hipEvent_t fork = nullptr, join = nullptr;
    hipError_t e = hipEventCreateWithFlags(&fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&join, hipEventDisableTiming);
    bool pending = false;
    int i = first_op;
    auto do_join = [&]() {
        if (!pending || e != hipSuccess) return;
        e = hipEventRecord(join, s2);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, join, 0);
        pending = false;
    };
    bool main_dirty = true;                                     // work issued on the main stream since the last fork
    for (; i <= last_op && e == hipSuccess; ++i) {
        const ftc_op& o = plan->ops[i];
        if (o.kind == FTC_OP_JOIN) { do_join(); continue; }
        if (o.flags & FTC_FLAG_SIDE_STREAM) {
            if (main_dirty) {
                e = hipEventRecord(fork, s);
                if (e == hipSuccess) e = hipStreamWaitEvent(s2, fork, 0);
                main_dirty = false;
            }
            if (e == hipSuccess) e = run_one(o, bases, s2);
            pending = true;
        } else {
            e = run_one(o, bases, s);
            main_dirty = true;
        }
    }
    const int failed = i - 1;
    hipError_t e_op = e;
    e = hipSuccess;
    do_join();
    if (fork) (void)hipEventDestroy(fork);
    if (join) (void)hipEventDestroy(join);
    if (e_op != hipSuccess || e != hipSuccess) {
        char buf[64];
        std::snprintf(buf, sizeof buf, "ftc_plan_run_streams: op %d", failed);
        return fail_hip(e_op != hipSuccess ? e_op : e, buf);
    }
    return FTC_OK;
}

int ftc_op_kernel_label(const ftc_op* op, char* buf, int len) {
    if (!op || !buf || len <= 0) return fail(FTC_ERR_INVALID, "ftc_op_kernel_label: null arguments");
    if (backbone::format_label(*op, buf, len)) return FTC_OK;      // STEM, DWCONV, SE, MBHEAD, FMBCONV, UPCAT: formatted from the choice (backbone_choice.h)
    if (op->kind == FTC_OP_CONV) conv_kernel_label(*op, buf, len);
    else if (op->kind == FTC_OP_WGRAD) wgrad_kernel_label(*op, buf, len);
    else if (!train::format_label(*op, buf, len)) return fail(FTC_ERR_INVALID, "ftc_op_kernel_label: unknown op kind");      // every other kind (train_choice.h)
    return FTC_OK;
}

int ftc_plan_profile(const ftc_plan* plan, void* const bases[FTC_NUM_BASES], void* stream, float* ms_out) {
    if (!plan || !bases || !ms_out) return fail(FTC_ERR_INVALID, "ftc_plan_profile: null arguments");
    const int n = (int)plan->ops.size();
    int rc = check_bases(plan, bases, 0, n - 1);
    if (rc != FTC_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<hipEvent_t> ev(n + 1);
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(FTC_ERR_HIP, "ftc_plan_profile: hipEventCreate failed");
    (void)hipEventRecord(ev[0], s);
    int ret = FTC_OK;
    for (int i = 0; i < n; ++i) {
        hipError_t e = run_one(plan->ops[i], bases, s);
        if (e != hipSuccess) { ret = fail_hip(e, "ftc_plan_profile: launch"); break; }
        (void)hipEventRecord(ev[i + 1], s);
    }
    hipError_t se = hipStreamSynchronize(s);
    if (ret == FTC_OK && se != hipSuccess) ret = fail_hip(se, "ftc_plan_profile: sync");
    if (ret == FTC_OK)
        for (int i = 0; i < n; ++i) (void)hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]);
    for (auto& e : ev) (void)hipEventDestroy(e);
    return ret;
}

int ftc_glyph_select(const float* logits0, const float* logits1, const float* logits2, int64_t ld0, int64_t ld1, int64_t ld2, int n,
                     float* soft0, float* soft1, float* soft2, int64_t* ids, float* probs, void* stream) {
    if (n < 0) return fail(FTC_ERR_INVALID, "ftc_glyph_select: n < 0");
    if (ld0 < 1091 || ld1 < 1093 || ld2 < 1097) return fail(FTC_ERR_INVALID, "ftc_glyph_select: row pitch ld_k must be >= m_k (1091, 1093, 1097)");
    if (n == 0) return FTC_OK;
    if (!logits0 || !logits1 || !logits2 || !ids || !probs) return fail(FTC_ERR_INVALID, "ftc_glyph_select: null pointer argument");
    hipError_t e = ftc_glyph_select_launch(logits0, logits1, logits2, ld0, ld1, ld2, n, soft0, soft1, soft2, ids, probs, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_glyph_select");
    return FTC_OK;
}

int ftc_decode(const float* heatmap, const float* features, int B, int h, int w, int C, const ftc_tile* tiles_dev,
               float logit_cut, int scale, int max_boxes, float* boxes, int box_stride, float* feats, int feat_stride,
               int32_t* index, int32_t* counts, void* scratch_dev, void* stream) {
    if (!heatmap || !features || !tiles_dev || !boxes || !feats || !index || !counts || !scratch_dev)
        return fail(FTC_ERR_INVALID, "ftc_decode: null pointer argument");
    if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || (C & 3) || max_boxes <= 0 || scale <= 0)
        return fail(FTC_ERR_INVALID, "ftc_decode: bad sizes (C must be a multiple of 4)");
    if ((long)h * w > 0x7fffffffL / 16) return fail(FTC_ERR_INVALID, "ftc_decode: map too large");
    if (box_stride < 9 || feat_stride < C || (feat_stride & 3) || (reinterpret_cast<uintptr_t>(feats) & 15) || (reinterpret_cast<uintptr_t>(features) & 15))
        return fail(FTC_ERR_INVALID, "ftc_decode: box_stride >= 9, feat_stride >= C and a multiple of 4 floats, feature rows 16-byte aligned");
    hipError_t e = launch_decode(heatmap, features, B, h, w, C, tiles_dev, logit_cut, scale, max_boxes, boxes, box_stride, feats,
                                 feat_stride, index, counts, scratch_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_decode");
    return FTC_OK;
}

int ftc_tile_gather(const unsigned char* page_u8, int page_h, int page_w, const int32_t* origins_yx_dev, int B, int tile_h,
                    int tile_w, float* tiles_out, void* stream) {
    if (!page_u8 || !origins_yx_dev || !tiles_out) return fail(FTC_ERR_INVALID, "ftc_tile_gather: null pointer argument");
    if (page_h <= 0 || page_w <= 0 || B <= 0 || tile_h <= 0 || tile_w <= 0) return fail(FTC_ERR_INVALID, "ftc_tile_gather: bad sizes");
    hipError_t e = launch_tile_gather(page_u8, page_h, page_w, origins_yx_dev, B, tile_h, tile_w, tiles_out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_tile_gather");
    return FTC_OK;
}

int ftc_paste_maps(const float* heatmap, const ftc_tile* tiles_dev, int B, int h, int w, int scale, float* canvases, int page_mh,
                   int page_mw, void* stream) {
    if (!heatmap || !tiles_dev || !canvases) return fail(FTC_ERR_INVALID, "ftc_paste_maps: null pointer argument");
    if (B <= 0 || h <= 0 || w <= 0 || scale <= 0 || page_mh <= 0 || page_mw <= 0) return fail(FTC_ERR_INVALID, "ftc_paste_maps: bad sizes");
    hipError_t e = launch_paste_maps(heatmap, tiles_dev, B, h, w, scale, canvases, page_mh, page_mw, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_paste_maps");
    return FTC_OK;
}

namespace {
// scratch of ftc_page_merge: header | kept boxes [N][4] f64 + their source rows (sequential fallback, result list) | rank-ordered edge table
// [N][6] f64 | status, neighbour counts / offsets, fill cursors | neighbour lists | a coverage bit image as large as the page
struct PageScratch { int64_t hdr, kept, keep_idx, rb, status, cnt, cursor, fill, fill_words, nbr, nbr_cap, total; };
PageScratch page_scratch_layout(int64_t n, int64_t page_h, int64_t page_w) {
    PageScratch L{};
    auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    int64_t o = 0;
    L.hdr = o; o += 256;
    L.kept = o; o = up(o + n * 32);
    L.keep_idx = o; o = up(o + n * 4);
    L.rb = o; o = up(o + n * 48);
    L.status = o; o = up(o + n * 4);
    L.cnt = o; o = up(o + (n + 1) * 4);
    L.cursor = o; o = up(o + (n + 1) * 4);
    L.fill_words = page_h * page_w / 32 + 64;
    L.fill = o; o = up(o + L.fill_words * 4);
    L.nbr = o;                                                   // the neighbour lists take the rest of the block
    int64_t cap = n * 256;                                       // default: room for 256 earlier overlapping candidates per box on average
    if (cap < (1 << 20)) cap = 1 << 20;
    if (cap > (1ll << 28)) cap = 1ll << 28;
    L.nbr_cap = cap;
    o = up(o + L.nbr_cap * 4);
    L.total = o;
    return L;
}
}  // namespace

int64_t ftc_page_merge_scratch_bytes(int n_boxes, int page_h, int page_w) {
    if (n_boxes <= 0 || page_h <= 0 || page_w <= 0) return 0;
    return page_scratch_layout(n_boxes, page_h, page_w).total;
}

int64_t ftc_page_order_scratch_bytes(int n_boxes) { return n_boxes > 0 ? 256 + (int64_t)n_boxes * 16 : 0; }

int ftc_page_order(const float* locations, int n_boxes, const double* hist0, float cut_off, int32_t* order_out, double* threshold_out, void* scratch,
                   int64_t scratch_bytes, void* stream) {
    if (!locations || !hist0 || !order_out || !threshold_out || !scratch) return fail(FTC_ERR_INVALID, "ftc_page_order: null pointer argument");
    if (n_boxes <= 0 || n_boxes > (1 << 20)) return fail(FTC_ERR_INVALID, "ftc_page_order: bad sizes");
    if (scratch_bytes < ftc_page_order_scratch_bytes(n_boxes)) return fail(FTC_ERR_INVALID, "ftc_page_order: scratch smaller than ftc_page_order_scratch_bytes");
    hipError_t e = launch_page_order(locations, n_boxes, hist0, cut_off, order_out, threshold_out, scratch, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_page_order");
    return FTC_OK;
}

int ftc_box_hists(const float* locations, int n_boxes, const float* page, int page_h, int page_w, float cut_off, double* hist_out,
                  void* stream) {
    if (!locations || !page || !hist_out) return fail(FTC_ERR_INVALID, "ftc_box_hists: null pointer argument");
    if (n_boxes <= 0 || page_h <= 0 || page_w <= 0) return fail(FTC_ERR_INVALID, "ftc_box_hists: bad sizes");
    hipError_t e = launch_box_hists(locations, n_boxes, page, page_h, page_w, cut_off, hist_out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_box_hists");
    return FTC_OK;
}

int ftc_page_merge_variant(const float* locations, const int32_t* order, int n_boxes, const double* hist1, const double* threshold_dev,
                           float cut_off, const float* seps, const float* codes, int mh, int mw, int scale, int page_h, int page_w, int variant,
                           int seed_start, double seed_scale, float* out_locations, int32_t* out_index, float* out_code_max, int32_t* out_count,
                           void* scratch, int64_t scratch_bytes, void* stream) {
    if (!locations || !order || !seps || !codes || !out_locations || !out_index || !out_count || !scratch)
        return fail(FTC_ERR_INVALID, "ftc_page_merge: null pointer argument");
    if (variant != FTC_PAGE_MERGE_PRODUCTION && variant != FTC_PAGE_MERGE_DEMO) return fail(FTC_ERR_INVALID, "ftc_page_merge: unknown variant");
    if (variant == FTC_PAGE_MERGE_PRODUCTION && (!hist1 || !threshold_dev)) return fail(FTC_ERR_INVALID, "ftc_page_merge: the production variant needs hist1 and threshold_dev");
    if (variant == FTC_PAGE_MERGE_PRODUCTION && seed_start >= 0 && seed_start < n_boxes) return fail(FTC_ERR_INVALID, "ftc_page_merge: seed rows exist only in the demo variant");
    if (n_boxes <= 0 || mh <= 0 || mw <= 0 || scale <= 0 || page_h <= 0 || page_w <= 0) return fail(FTC_ERR_INVALID, "ftc_page_merge: bad sizes");
    if (n_boxes > (1 << 20)) return fail(FTC_ERR_INVALID, "ftc_page_merge: more than 2^20 boxes");
    // fixed part | coverage image of the page | neighbour lists: whatever the block has behind the image (ftc_page_merge_scratch_bytes leaves
    // room for 256 per box).  A page whose lists do not fit goes through the sequential kernel on the device: same result, slower.
    const PageScratch lay = page_scratch_layout(n_boxes, page_h, page_w);
    if (scratch_bytes < lay.nbr + 4096) return fail(FTC_ERR_INVALID, "ftc_page_merge: scratch smaller than the fixed part of ftc_page_merge_scratch_bytes");
    const int64_t nbr_cap = (scratch_bytes - lay.nbr) / 4;
    char* sp = static_cast<char*>(scratch);
    const char* fs_env = std::getenv("FTC_PAGE_MERGE_SEQ");                  // A/B and tests: "1" = the sequential (round-3) kernel
    const bool force_seq = fs_env && fs_env[0] == '1';
    hipError_t e = launch_greedy(locations, order, n_boxes, hist1, threshold_dev, cut_off, reinterpret_cast<double*>(sp + lay.kept),
                                 reinterpret_cast<int*>(sp + lay.keep_idx), reinterpret_cast<int*>(sp + lay.hdr), reinterpret_cast<double*>(sp + lay.rb),
                                 reinterpret_cast<int*>(sp + lay.status), reinterpret_cast<int*>(sp + lay.cnt), reinterpret_cast<int*>(sp + lay.cursor),
                                 reinterpret_cast<int*>(sp + lay.nbr), (long)nbr_cap, reinterpret_cast<unsigned int*>(sp + lay.fill), (long)lay.fill_words,
                                 force_seq ? 1 : 0, seps, codes, mh, mw, scale, out_locations, out_index, out_count, variant, seed_start, seed_scale,
                                 out_code_max, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_page_merge");
    return FTC_OK;
}

int ftc_page_merge(const float* locations, const int32_t* order, int n_boxes, const double* hist1, const double* threshold_dev,
                   float cut_off, const float* seps, const float* codes, int mh, int mw, int scale, int page_h, int page_w, float* out_locations,
                   int32_t* out_index, int32_t* out_count, void* scratch, int64_t scratch_bytes, void* stream) {
    return ftc_page_merge_variant(locations, order, n_boxes, hist1, threshold_dev, cut_off, seps, codes, mh, mw, scale, page_h, page_w,
                                  FTC_PAGE_MERGE_PRODUCTION, -1, 1.0, out_locations, out_index, nullptr, out_count, scratch, scratch_bytes, stream);
}

int ftc_adamw_schedulefree_step(const ftc_mt_chunk* chunks_dev, int n_chunks, float beta2, float one_minus_beta2, float bias_correction2,
                                float eps, float weight_decay, float ckp1, float y_alpha, float lr, int write_grad, void* stream) {
    if (!chunks_dev || n_chunks <= 0) return fail(FTC_ERR_INVALID, "ftc_adamw_schedulefree_step: empty chunk table");
    if (!(bias_correction2 > 0.0f)) return fail(FTC_ERR_INVALID, "ftc_adamw_schedulefree_step: bias_correction2 must be positive");
    hipError_t e = launch_adamw_sf(chunks_dev, n_chunks, beta2, one_minus_beta2, bias_correction2, eps, weight_decay, ckp1, y_alpha, lr,
                                   write_grad, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_adamw_schedulefree_step");
    return FTC_OK;
}

int ftc_topk_mask(const float* values, int64_t n, int64_t k, unsigned char* mask, int32_t* sel_index, int32_t* count, void* stream) {
    if (!values || !mask) return fail(FTC_ERR_INVALID, "ftc_topk_mask: null pointer argument");
    if (n <= 0 || n >= 0x7fffffffL || k < 0) return fail(FTC_ERR_INVALID, "ftc_topk_mask: need 0 < n < 2^31 and k >= 0");
    hipError_t e = launch_topk_mask(values, (long)n, (long)k, mask, sel_index, count, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_topk_mask");
    return FTC_OK;
}

int ftc_mask_compact(const unsigned char* mask, int64_t n, int32_t* sel_index, int64_t cap, int32_t* count, void* stream) {
    if (!mask || !sel_index || !count) return fail(FTC_ERR_INVALID, "ftc_mask_compact: null pointer argument");
    if (n <= 0 || n >= 0x7fffffffL || cap < 0) return fail(FTC_ERR_INVALID, "ftc_mask_compact: need 0 < n < 2^31 and cap >= 0");
    hipError_t e = launch_mask_compact(mask, (long)n, sel_index, (long)cap, count, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_mask_compact");
    return FTC_OK;
}

int ftc_gather_rows(const float* features, const int32_t* sel_index, const int32_t* count, int64_t cap, int C, int c_pad, void* rows,
                    int out_dtype, void* stream) {
    if (!features || !sel_index || !rows) return fail(FTC_ERR_INVALID, "ftc_gather_rows: null pointer argument");
    if (cap <= 0 || C <= 0 || (C & 3) || c_pad < C || (c_pad & 7) || (out_dtype != FTC_F32 && !ftc_is16(out_dtype)))
        return fail(FTC_ERR_INVALID, "ftc_gather_rows: need cap > 0, C % 4 == 0, c_pad >= C, c_pad % 8 == 0, out_dtype fp32 | bf16 | fp16");
    hipError_t e = launch_gather_rows(features, sel_index, count, (long)cap, C, c_pad, rows, out_dtype, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_gather_rows");
    return FTC_OK;
}

int ftc_pack_train_weights(const ftc_pack_entry* entries_dev, int n_entries, int64_t max_elems, void* stream) {
    if (!entries_dev || n_entries <= 0 || n_entries > 65535 || max_elems <= 0) return fail(FTC_ERR_INVALID, "ftc_pack_train_weights: need 1..65535 entries and max_elems > 0");
    hipError_t e = launch_pack_train(entries_dev, n_entries, (long)max_elems, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_pack_train_weights");
    return FTC_OK;
}

int ftc_wgrad_splits(int B, int Ho, int Wo, int Cout, int Cin, int ksize) {
    if (B <= 0 || Ho <= 0 || Wo <= 0 || Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3)) return 1;
    return ftc_wgrad_splits_impl(B, Ho, Wo, Cout, Cin, ksize);
}

int ftc_op_extents(const ftc_op* op, int64_t bytes[FTC_NUM_OPERANDS], int32_t state[FTC_NUM_OPERANDS]) {
    if (!op || !bytes || !state) return fail(FTC_ERR_INVALID, "ftc_op_extents: null arguments");
    OpExtents e;
    if (const char* refused = op_extents(*op, &e)) return fail(FTC_ERR_INVALID, std::string("ftc_op_extents: ") + refused);
    std::memcpy(bytes, e.bytes, sizeof e.bytes);
    std::memcpy(state, e.state, sizeof e.state);
    return FTC_OK;
}

int64_t ftc_losses_scratch_bytes(void) { return FTC_LOSSES_SCRATCH_BYTES; }

int ftc_losses(const float* heatmap, const int64_t heat_strides[4], const float* labelmap, const int32_t* idmap, int B, int h, int w,
               const float* dec0, const float* dec1, const float* dec2, const int32_t* sel_index, const int32_t* count, int64_t cap,
               float* out, void* scratch, void* stream) {
    if (!heatmap || !heat_strides || !labelmap || !idmap || !out || !scratch) return fail(FTC_ERR_INVALID, "ftc_losses: null pointer argument");
    if (B <= 0 || h <= 0 || w <= 0) return fail(FTC_ERR_INVALID, "ftc_losses: bad sizes");
    const bool has_dec = dec0 || dec1 || dec2;
    if (has_dec && (!dec0 || !dec1 || !dec2 || !sel_index || !count || cap <= 0)) return fail(FTC_ERR_INVALID, "ftc_losses: decoder outputs need all three heads, sel_index, count and cap > 0");
    const long hs[4] = {(long)heat_strides[0], (long)heat_strides[1], (long)heat_strides[2], (long)heat_strides[3]};
    const float* dec[3] = {dec0, dec1, dec2};
    static const int mod[3] = {1091, 1093, 1097};                   // util_func.py:5 modulo_list
    hipError_t e = launch_losses(heatmap, hs, labelmap, idmap, B, h, w, has_dec ? dec : nullptr, mod, sel_index, count, (long)cap, out, scratch,
                                 static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_losses");
    return FTC_OK;
}

int ftc_cov_weighting_step(const float* losses, int n, int iteration, float* state, float* out_loss, void* stream) {
    if (!losses || !state || !out_loss) return fail(FTC_ERR_INVALID, "ftc_cov_weighting_step: null pointer argument");
    if (n <= 0 || n > 16 || iteration < 0) return fail(FTC_ERR_INVALID, "ftc_cov_weighting_step: need 0 < n <= 16 and iteration >= 0");
    hipError_t e = launch_cov_step(losses, n, iteration, state, out_loss, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "ftc_cov_weighting_step");
    return FTC_OK;
}

}  // extern "C"
