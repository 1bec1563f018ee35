// Self-contained model entry points of the C ABI (include/ftc.h): ftc_create / ftc_forward / ftc_destroy, the decoder entry points and the
// plan inspection calls.  Everything a host needs to run the detector path lives behind them, in the library: the network description
// (model_net.h), the weight packing (pack.hip) and the plan builder (plan.hip); this file holds the model object's plan caches.
// Host-only code: no kernels here.
#include <cstring>
#include <new>

#include "model_net.h"

using namespace ftc_model_detail;

namespace {

// every op of a plan the library built goes through the same validation as a caller-supplied op list
int validate_plan(const ModelPlan& mp) {
    ftc_plan* checked = nullptr;
    const int rc = ftc_plan_create(mp.plan.ops.data(), (int)mp.plan.ops.size(), mp.plan.workspace_bytes, mp.plan.weights_bytes, &checked);
    if (rc == FTC_OK) ftc_plan_destroy(checked);
    return rc;
}

// The detector plan for a shape, under the plan switches as the environment sets them at this call (the cache is keyed by both)
int get_plan(ftc_model* m, int B, int H, int W, int nchw, ModelPlan** out) {
    if (!m) return ftc_set_error(FTC_ERR_INVALID, "ftc model: null handle");
    if (B <= 0 || H <= 0 || W <= 0 || (H % 32) || (W % 32))
        return ftc_set_error(FTC_ERR_INVALID, "ftc model: B must be positive and H, W positive multiples of 32 (the reference always uses 768)");
    const PlanKey key{B, H, W, nchw ? 1 : 0, read_plan_options()};
    std::lock_guard<std::mutex> lk(m->mu);
    auto it = m->plans.find(key);
    if (it == m->plans.end()) {
        std::unique_ptr<ModelPlan> mp(new (std::nothrow) ModelPlan());
        if (!mp) return ftc_set_error(FTC_ERR_NOMEM, "ftc model: out of host memory");
        int rc = build_model_plan(m, B, H, W, nchw != 0, key.opt, mp.get());
        if (rc == FTC_OK) rc = validate_plan(*mp);
        if (rc != FTC_OK) return rc;
        it = m->plans.emplace(key, std::move(mp)).first;
    }
    *out = it->second.get();
    return FTC_OK;
}

}  // namespace

extern "C" {

int ftc_create(const ftc_tensor* tensors, int n_tensors, const char* model_size, int precision, ftc_model** out) {
    if (!tensors || n_tensors <= 0 || !out) return ftc_set_error(FTC_ERR_INVALID, "ftc_create: null/empty arguments");
    const std::string size = model_size && *model_size ? model_size : "xl";
    if (stage_rows(size).empty()) return ftc_set_error(FTC_ERR_INVALID, "ftc_create: model_size must be one of xl, l, m, s");
    if (precision != FTC_F32 && precision != FTC_BF16 && precision != FTC_F16 && precision != FTC_PRECISION_F16X3)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_create: precision must be FTC_F32, FTC_BF16, FTC_F16 or FTC_PRECISION_F16X3");
    const int split16 = precision == FTC_PRECISION_F16X3 ? 1 : 0;
    if (split16) precision = FTC_F32;
    Weights w;
    for (int i = 0; i < n_tensors; ++i) {
        const ftc_tensor& t = tensors[i];
        if (!t.name || !t.data) return ftc_set_error(FTC_ERR_INVALID, "ftc_create: tensor " + std::to_string(i) + " has a null name or data pointer");
        if (t.dtype != FTC_F32) continue;                               // e.g. num_batches_tracked (int64): not used by the forward pass
        if (t.ndim < 0 || t.ndim > 4) return ftc_set_error(FTC_ERR_INVALID, std::string("ftc_create: tensor '") + t.name + "' has more than 4 dimensions");
        std::string name = t.name;
        if (name.rfind("detector.", 0) == 0) name = name.substr(9);     // TextDetectorModel keys ("decoder.*" keep their prefix)
        TensorView v;
        v.data = static_cast<const float*>(t.data);
        v.shape.assign(t.shape, t.shape + t.ndim);
        w.t[name] = v;
    }
    ftc_model* m = new (std::nothrow) ftc_model();
    if (!m) return ftc_set_error(FTC_ERR_NOMEM, "ftc_create: out of host memory");
    m->size = size;
    m->precision = precision;
    m->split16 = split16;
    const int rc = pack_weights(m, w);
    if (rc != FTC_OK) { delete m; return rc; }
    *out = m;
    return FTC_OK;
}

void ftc_destroy(ftc_model* model) { delete model; }

int64_t ftc_weights_bytes(const ftc_model* model) { return model ? (int64_t)model->blob.bytes.size() : 0; }

const void* ftc_weights_host(const ftc_model* model) { return model ? model->blob.bytes.data() : nullptr; }

int64_t ftc_weights_offset(const ftc_model* model, const char* name) {
    if (!model || !name) return -1;
    auto it = model->blob.table.find(name);
    return it == model->blob.table.end() ? -1 : it->second;
}

int64_t ftc_workspace_bytes(ftc_model* model, int B, int H, int W) {
    ModelPlan* mp = nullptr;
    if (get_plan(model, B, H, W, 0, &mp) != FTC_OK) return -1;
    return mp->plan.workspace_bytes;
}

int ftc_forward(ftc_model* model, const void* weights_dev, const void* image, int B, int H, int W, int nchw, int with_nms, void* heatmap,
                void* features, void* workspace, void* stream) {
    if (!weights_dev || !image || !heatmap || !features || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_forward: null pointer argument");
    ModelPlan* mp = nullptr;
    int rc = get_plan(model, B, H, W, nchw, &mp);
    if (rc != FTC_OK) return rc;
    void* bases[FTC_NUM_BASES] = {nullptr, workspace, const_cast<void*>(weights_dev), const_cast<void*>(image), heatmap, features};
    const int n = (int)mp->plan.ops.size();
    return ftc_plan_run(&mp->plan, bases, stream, 0, with_nms ? n - 1 : n - 2);
}

static int get_decoder_plan(ftc_model* m, int n_rows, std::shared_ptr<ModelPlan>* out, bool glyph = false) {
    if (!m) return ftc_set_error(FTC_ERR_INVALID, "ftc decoder: null model");
    if (!m->has_decoder) return ftc_set_error(FTC_ERR_INVALID, "ftc decoder: the model was created from a checkpoint without decoder.* tensors");
    if (n_rows <= 0) return ftc_set_error(FTC_ERR_INVALID, "ftc decoder: n_rows must be positive");
    std::lock_guard<std::mutex> lk(m->mu);
    PlanLru& cache = glyph ? m->glyph_plans : m->decoder_plans;
    const PlanOptions opt = read_plan_options();
    if (glyph && m->glyph_pins.empty()) {
        ModelPlan ref;
        int rc = build_decoder_plan(m, ftc_model::kGlyphPinRows, opt, &ref);
        if (rc != FTC_OK) return rc;
        for (const ftc_op& o : ref.plan.ops) m->glyph_pins.push_back(o.kind == FTC_OP_CONV ? conv_pinned_choice(o) : o.aux0);
    }
    *out = cache.find(n_rows);
    if (*out) return FTC_OK;
    std::shared_ptr<ModelPlan> mp(new (std::nothrow) ModelPlan());
    if (!mp) return ftc_set_error(FTC_ERR_NOMEM, "ftc decoder: out of host memory");
    int rc = build_decoder_plan(m, n_rows, opt, mp.get());
    if (rc != FTC_OK) return rc;
    if (glyph) {
        if (mp->plan.ops.size() != m->glyph_pins.size()) return ftc_set_error(FTC_ERR_INVALID, "ftc glyph decode: decoder plans differ in length");
        for (size_t i = 0; i < mp->plan.ops.size(); ++i) mp->plan.ops[i].aux0 = m->glyph_pins[i];
    }
    rc = validate_plan(*mp);
    if (rc != FTC_OK) return rc;
    cache.insert(n_rows, mp);
    *out = mp;
    return FTC_OK;
}

// ftc_glyph_decode pads the batch to 64 * 2^k or 96 * 2^k rows (at most 1.5x the work of the rows themselves)
static int64_t glyph_bucket(int n) {
    for (int64_t b = 64;; b *= 2) {
        if (n <= b) return b;
        if (n <= b * 3 / 2) return b * 3 / 2;
    }
}

namespace {
constexpr int kGlyphMod[3] = {1091, 1093, 1097};          // util_func.py:5 modulo_list
int64_t align256(int64_t v) { return (v + 255) & ~int64_t(255); }
struct GlyphLayout { int64_t rows, logits[3], plan, total; };
GlyphLayout glyph_layout(const ftc_model* m, int64_t bucket, int64_t plan_ws) {
    GlyphLayout g;
    int64_t off = 0;
    g.rows = off; off += align256(bucket * 128 * (m->precision == FTC_F32 ? 4 : 2));
    for (int k = 0; k < 3; ++k) { g.logits[k] = off; off += align256(bucket * kGlyphMod[k] * 4); }
    g.plan = off; off += align256(plan_ws);
    g.total = off;
    return g;
}
}  // namespace

int64_t ftc_decoder_workspace_bytes(ftc_model* model, int n_rows) {
    std::shared_ptr<ModelPlan> mp;
    if (get_decoder_plan(model, n_rows, &mp) != FTC_OK) return -1;
    return mp->plan.workspace_bytes;
}

int ftc_decoder_forward(ftc_model* model, const void* weights_dev, const void* rows, int n_rows, float* out0, float* out1, float* out2,
                        void* workspace, void* stream) {
    if (!weights_dev || !rows || !out0 || !out1 || !out2 || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_decoder_forward: null pointer argument");
    std::shared_ptr<ModelPlan> mp;
    int rc = get_decoder_plan(model, n_rows, &mp);
    if (rc != FTC_OK) return rc;
    float* outs[3] = {out0, out1, out2};
    for (int i = 0; i < 3; ++i) {
        void* bases[FTC_NUM_BASES] = {nullptr, workspace, const_cast<void*>(weights_dev), const_cast<void*>(rows), outs[i], nullptr};
        rc = ftc_plan_run(&mp->plan, bases, stream, 3 * i, 3 * i + 2);
        if (rc != FTC_OK) return rc;
    }
    return FTC_OK;
}

int64_t ftc_glyph_decode_workspace_bytes(ftc_model* model, int n_rows) {
    if (n_rows < 0) { ftc_set_error(FTC_ERR_INVALID, "ftc_glyph_decode_workspace_bytes: n_rows < 0"); return -1; }
    if (n_rows == 0) return 0;
    if (n_rows > (1 << 24)) { ftc_set_error(FTC_ERR_INVALID, "ftc_glyph_decode_workspace_bytes: more than 2^24 rows (split the batch)"); return -1; }
    const int64_t bucket = glyph_bucket(n_rows);
    std::shared_ptr<ModelPlan> mp;
    if (get_decoder_plan(model, (int)bucket, &mp, true) != FTC_OK) return -1;
    return glyph_layout(model, bucket, mp->plan.workspace_bytes).total;
}

int ftc_glyph_decode(ftc_model* model, const void* weights_dev, const void* rows, int n_rows, int64_t* ids, float* probs,
                     float* soft0, float* soft1, float* soft2, void* workspace, void* stream) {
    if (!model) return ftc_set_error(FTC_ERR_INVALID, "ftc_glyph_decode: null model");
    if (n_rows < 0) return ftc_set_error(FTC_ERR_INVALID, "ftc_glyph_decode: n_rows < 0");
    if (n_rows > (1 << 24)) return ftc_set_error(FTC_ERR_INVALID, "ftc_glyph_decode: more than 2^24 rows (split the batch)");
    if (!model->has_decoder) return ftc_set_error(FTC_ERR_INVALID, "ftc decoder: the model was created from a checkpoint without decoder.* tensors");
    if (n_rows == 0) return FTC_OK;
    if (!weights_dev || !rows || !ids || !probs || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_glyph_decode: null pointer argument");
    const int64_t bucket = glyph_bucket(n_rows);
    std::shared_ptr<ModelPlan> mp;
    int rc = get_decoder_plan(model, (int)bucket, &mp, true);
    if (rc != FTC_OK) return rc;
    const GlyphLayout g = glyph_layout(model, bucket, mp->plan.workspace_bytes);
    char* ws = static_cast<char*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the bucket's rows: the caller's n_rows, zeros after them (the plan reads `bucket` rows)
    const int64_t row_bytes = 128 * (model->precision == FTC_F32 ? 4 : 2);
    hipError_t e = hipMemcpyAsync(ws + g.rows, rows, (size_t)(n_rows * row_bytes), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && bucket > n_rows) e = hipMemsetAsync(ws + g.rows + n_rows * row_bytes, 0, (size_t)((bucket - n_rows) * row_bytes), s);
    if (e != hipSuccess) return ftc_set_error(FTC_ERR_HIP, std::string("ftc_glyph_decode: ") + hipGetErrorString(e));
    for (int i = 0; i < 3; ++i) {
        void* bases[FTC_NUM_BASES] = {nullptr, ws + g.plan, const_cast<void*>(weights_dev), ws + g.rows, ws + g.logits[i], nullptr};
        rc = ftc_plan_run(&mp->plan, bases, stream, 3 * i, 3 * i + 2);
        if (rc != FTC_OK) return rc;
    }
    e = ftc_glyph_select_launch(reinterpret_cast<const float*>(ws + g.logits[0]), reinterpret_cast<const float*>(ws + g.logits[1]),
                                reinterpret_cast<const float*>(ws + g.logits[2]), kGlyphMod[0], kGlyphMod[1], kGlyphMod[2], n_rows,
                                soft0, soft1, soft2, ids, probs, s);
    if (e != hipSuccess) return ftc_set_error(FTC_ERR_HIP, std::string("ftc_glyph_decode: select launch: ") + hipGetErrorString(e));
    return FTC_OK;
}

int ftc_model_plan(ftc_model* model, int B, int H, int W, int nchw, const ftc_plan** plan, ftc_plan_info* info) {
    ModelPlan* mp = nullptr;
    int rc = get_plan(model, B, H, W, nchw, &mp);
    if (rc != FTC_OK) return rc;
    if (plan) *plan = &mp->plan;
    if (info) {
        info->n_ops = (int)mp->plan.ops.size();
        info->map_h = mp->h; info->map_w = mp->w;
        info->reserved = 0;
        info->workspace_bytes = mp->plan.workspace_bytes;
        info->weights_bytes = mp->plan.weights_bytes;
        info->peak_live_bytes = mp->peak_live_bytes;
        info->total_buffer_bytes = mp->total_buffer_bytes;
    }
    return FTC_OK;
}

int ftc_model_op_info(ftc_model* model, int B, int H, int W, int nchw, int index, ftc_op_info* out) {
    ModelPlan* mp = nullptr;
    int rc = get_plan(model, B, H, W, nchw, &mp);
    if (rc != FTC_OK) return rc;
    if (!out || index < 0 || index >= (int)mp->meta.size()) return ftc_set_error(FTC_ERR_INVALID, "ftc_model_op_info: index out of range");
    const OpMeta& me = mp->meta[index];
    std::memset(out, 0, sizeof *out);
    std::strncpy(out->name, me.name.c_str(), sizeof out->name - 1);
    std::strncpy(out->kind, me.kind.c_str(), sizeof out->kind - 1);
    out->flops = me.flops;
    out->bytes = me.bytes;
    return FTC_OK;
}

int ftc_plan_op(const ftc_plan* plan, int index, ftc_op* out) {
    if (!plan || !out || index < 0 || index >= (int)plan->ops.size()) return ftc_set_error(FTC_ERR_INVALID, "ftc_plan_op: bad arguments");
    *out = plan->ops[index];
    return FTC_OK;
}

}  // extern "C"
