// Host-only definitions shared by the three translation units behind ftc_create / ftc_forward (include/ftc.h):
//   pack.hip   the weight packing (once per checkpoint): eval-mode BatchNorm folded into the preceding convolution in float64,
//              K-major [Cout][kh*kw][Cin] re-layout, conversion to the MFMA compute type, one blob
//   plan.hip   the plan builder (once per input shape and switch setting): the plan switches, the per-shape op list with its
//              liveness-based activation arena, and the measured kernel selection (the table key and the lookup, also exported for a
//              caller's own op array: ftc_conv_signature, ftc_tune_ops)
//   model.hip  ftc_model, the plan caches and the extern "C" entry points of the model
// and the network description all of them read (what the reference expresses as nn.Module composition -- CenterNetDetection.forward,
// models/detector.py:217-230 = stem + 100 Fused-MBConv / MBConv blocks with taps (BackboneModel.forward :139-146,
// config rows :12-28) + nine Leafmap heads (:148-201) -- followed by the NMS of CenterNetDetector.forward (:289-296)).
#pragma once
#include <algorithm>
#include <compare>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ftc_host.h"

namespace ftc_model_detail {

constexpr int64_t ALIGN = 256;
inline int64_t align_up(int64_t n, int64_t a = ALIGN) { return (n + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------------
// network description
// ------------------------------------------------------------------------------------------------
struct StageRow { bool fused; int expand, kernel, stride, cin, cout, layers; };
struct BlockSpec {
    bool fused;
    std::string prefix;      // "backbone.features.4.0"
    int cin, cout, exp, stride, squeeze;
    bool residual;
};
struct HeadSpec { const char* name; int out_dim; int ch0; };

// efficientnet_v2_xl (models/detector.py:12-28) and torchvision's published s/m/l tables (models/detector.py:131-136)
inline const std::vector<StageRow>& stage_rows(const std::string& size) {
    static const std::map<std::string, std::vector<StageRow>> t = {
        {"xl", {{true, 1, 3, 1, 32, 32, 4}, {true, 4, 3, 2, 32, 64, 8}, {true, 4, 3, 2, 64, 96, 8}, {false, 4, 3, 2, 96, 192, 16},
                {false, 6, 3, 1, 192, 256, 24}, {false, 6, 3, 2, 256, 512, 32}, {false, 6, 3, 1, 512, 640, 8}}},
        {"l", {{true, 1, 3, 1, 32, 32, 4}, {true, 4, 3, 2, 32, 64, 7}, {true, 4, 3, 2, 64, 96, 7}, {false, 4, 3, 2, 96, 192, 10},
               {false, 6, 3, 1, 192, 224, 19}, {false, 6, 3, 2, 224, 384, 25}, {false, 6, 3, 1, 384, 640, 7}}},
        {"m", {{true, 1, 3, 1, 24, 24, 3}, {true, 4, 3, 2, 24, 48, 5}, {true, 4, 3, 2, 48, 80, 5}, {false, 4, 3, 2, 80, 160, 7},
               {false, 6, 3, 1, 160, 176, 14}, {false, 6, 3, 2, 176, 304, 18}, {false, 6, 3, 1, 304, 512, 5}}},
        {"s", {{true, 1, 3, 1, 24, 24, 2}, {true, 4, 3, 2, 24, 48, 4}, {true, 4, 3, 2, 48, 64, 4}, {false, 4, 3, 2, 64, 128, 6},
               {false, 6, 3, 1, 128, 160, 9}, {false, 6, 3, 2, 160, 256, 15}}},
    };
    static const std::vector<StageRow> none;
    auto it = t.find(size);
    return it == t.end() ? none : it->second;
}
inline std::vector<int> tap_dims(const std::string& size) {
    if (size == "xl") return {64, 96, 256, 1280};
    if (size == "l") return {64, 96, 224, 1280};
    if (size == "m") return {48, 80, 176, 1280};
    return {48, 64, 160, 1280};
}
constexpr int LAST_CHANNEL = 1280, FPN_DIM = 192, FEATURE_DIM = 100;
constexpr double BACKBONE_BN_EPS = 1e-3, HEAD_BN_EPS = 1e-5;     // models/detector.py:27; nn.BatchNorm2d default (:161-184)
// CenterNetDetection heads in forward order (models/detector.py:207-230; the reference's spelling "sepatator")
constexpr int NHEADS = 9;
constexpr HeadSpec HEADS[NHEADS] = {{"keyheatmap", 1, 0}, {"sizes", 2, 1}, {"textline", 1, 3}, {"sepatator", 1, 4}, {"code1", 1, 5},
                                    {"code2", 1, 6}, {"code4", 1, 7}, {"code8", 1, 8}, {"feature", FEATURE_DIM, -1}};
constexpr int DECODER_MID = 2048, DECODER_KPAD = 128;
constexpr int DECODER_MODULO[3] = {1091, 1093, 1097};          // util_func.py:5 modulo_list

inline int make_divisible(double v, int d = 8) {        // torchvision _make_divisible
    int nv = std::max(d, (int)(v + d / 2.0) / d * d);
    if (nv < 0.9 * v) nv += d;
    return nv;
}

inline std::vector<std::vector<BlockSpec>> backbone_blocks(const std::string& size) {
    std::vector<std::vector<BlockSpec>> out;
    const auto& rows = stage_rows(size);
    for (size_t si = 0; si < rows.size(); ++si) {
        const StageRow& r = rows[si];
        std::vector<BlockSpec> st;
        for (int j = 0; j < r.layers; ++j) {
            const int bcin = j == 0 ? r.cin : r.cout, bstride = j == 0 ? r.stride : 1;
            st.push_back({r.fused, "backbone.features." + std::to_string(si + 1) + "." + std::to_string(j), bcin, r.cout,
                          make_divisible((double)bcin * r.expand), bstride, std::max(1, bcin / 4), bstride == 1 && bcin == r.cout});
        }
        out.push_back(st);
    }
    return out;
}

// ------------------------------------------------------------------------------------------------
// weights (pack.hip)
// ------------------------------------------------------------------------------------------------
struct TensorView {
    const float* data = nullptr;
    std::vector<int64_t> shape;
    int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

struct Weights {                    // the caller's checkpoint by name; `missing`: the first tensor that was absent or mis-shaped
    std::map<std::string, TensorView> t;
    std::string missing;
    const TensorView* get(const std::string& k, std::initializer_list<int64_t> shape);
};

struct Blob {                       // the packed weights: 256-byte aligned tensors by name
    std::vector<uint8_t> bytes;
    std::map<std::string, int64_t> table;
    uint8_t* add(const std::string& name, int64_t nbytes);
    void add_f32(const std::string& name, const double* v, int64_t n);
    void add_f32(const std::string& name, const float* v, int64_t n);
    // MFMA compute type: fp32, or bf16 / fp16 (double -> float -> 16 bit, both steps round-to-nearest-even), or pre-split fp16x3 chunks
    void add_compute(const std::string& name, const double* v, int64_t n, int dt);
    // fp16x3 packing: the first tensor given to add_compute that holds a value which is not finite or lies beyond +-65504.  The split would
    // clamp it silently (hi = +-65504, lo = 0) where the reference does not: pack_weights refuses the checkpoint and names the tensor.
    std::string out_of_range;
};

// ------------------------------------------------------------------------------------------------
// plans (plan.hip)
// ------------------------------------------------------------------------------------------------
// Every environment switch of plan construction, read in one place (read_plan_options) when a plan is asked for; the detector plan cache is
// keyed by them.  What each one does, its default and the modes it affects: DESIGN.md section 4, "Where a plan is decided, and its switches".
struct PlanOptions {
    bool no_mbslice = false, no_mbslice_x3 = false, no_mbband = false;                  // FTC_NO_MBSLICE, FTC_NO_MBSLICE_X3, FTC_NO_MBBAND
    bool mbslice_96 = true;                                                             // FTC_MBSLICE_96 (off when the value starts with '0')
    int mbslice_minwg = 128;                                                            // FTC_MBSLICE_MINWG (atoi)
    bool no_fmbfuse = false, no_fmbfuse_x3 = false, fmbfuse_all = false;                // FTC_NO_FMBFUSE, FTC_NO_FMBFUSE_X3, FTC_FMBFUSE_ALL
    bool no_kblock = false, no_x3fold = false, no_presplit = false;                     // FTC_NO_KBLOCK, FTC_NO_X3FOLD, FTC_NO_PRESPLIT
    bool no_topfuse = false, no_topfuse32 = false;                                      // FTC_NO_TOPFUSE, FTC_NO_TOPFUSE32
    bool no_upfuse = false, no_upfuse32 = false, no_upfuse32_l2 = false;                // FTC_NO_UPFUSE, FTC_NO_UPFUSE32, FTC_NO_UPFUSE32_L2
    bool no_bnfold = false, no_bnfold32 = false, no_wl1 = false, no_tuning = false;     // FTC_NO_BNFOLD, FTC_NO_BNFOLD32, FTC_NO_WL1, FTC_NO_TUNING
    int shrink_buf = -1;                                                                // FTC_PLAN_SHRINK_BUF (tests: that buffer is reserved 256 bytes short)
    auto operator<=>(const PlanOptions&) const = default;
};
// tuning_override: if given, receives the value of FTC_TUNING_OVERRIDE as it was at the first call in the process (or null)
PlanOptions read_plan_options(const char** tuning_override = nullptr);

struct OpMeta { std::string name, kind; double flops = 0, bytes = 0; };
struct ModelPlan {
    ftc_plan plan;
    std::vector<OpMeta> meta;
    int B, H, W, h, w;
    int64_t peak_live_bytes = 0, total_buffer_bytes = 0;
};

// Plans by row count.  The count follows the data (peaks per page), so the cache is bounded: at most kMax entries, the least recently
// used one is dropped (shared_ptr: a caller that is still running the evicted plan keeps it alive).
// (an entry is evicted when a newly built plan is inserted, so a failed build evicts nothing; each cache has its own clock)
struct PlanLru {
    static constexpr size_t kMax = 16;
    std::map<int, std::shared_ptr<ModelPlan>> plans;
    std::map<int, uint64_t> use;
    uint64_t clock = 0;
    std::shared_ptr<ModelPlan> find(int rows) {
        auto it = plans.find(rows);
        if (it == plans.end()) return nullptr;
        use[rows] = ++clock;
        return it->second;
    }
    void insert(int rows, std::shared_ptr<ModelPlan> p) {
        if (plans.size() >= kMax) {
            auto lru = use.begin();
            for (auto u = use.begin(); u != use.end(); ++u)
                if (u->second < lru->second) lru = u;
            plans.erase(lru->first);
            use.erase(lru);
        }
        plans[rows] = std::move(p);
        use[rows] = ++clock;
    }
};

struct PlanKey {
    int B, H, W, nchw;
    PlanOptions opt;
    auto operator<=>(const PlanKey&) const = default;
};

}  // namespace ftc_model_detail

struct ftc_model {
    using Blob = ftc_model_detail::Blob;
    using PlanKey = ftc_model_detail::PlanKey;
    using ModelPlan = ftc_model_detail::ModelPlan;
    using PlanLru = ftc_model_detail::PlanLru;
    std::string size;
    int precision;                          // FTC_F32 | FTC_BF16 | FTC_F16
    int split16 = 0;                        // FTC_PRECISION_F16X3: the fp32 plan with FTC_FLAG_SPLIT16 on every convolution
    Blob blob;
    bool has_decoder = false;               // the checkpoint carried the "decoder.*" tensors (SimpleDecoder)
    std::mutex mu;
    std::map<PlanKey, std::unique_ptr<ModelPlan>> plans;
    // The two decoder caches are keyed by rows alone.  Of the switches only FTC_NO_TUNING reaches a decoder plan (as it was when the plan was
    // first built), and the glyph plans run pinned kernel choices that are taken once per model by design.
    PlanLru decoder_plans;
    // ftc_glyph_decode: decoder plans by row BUCKET, every one running the GEMM kernel choices of `glyph_pins` (one aux0 per op, taken
    // from the plan of kGlyphPinRows rows) -- a row's logits then do not depend on the batch it came in.
    PlanLru glyph_plans;
    std::vector<int> glyph_pins;
    static constexpr int kGlyphPinRows = 8192;
};

namespace ftc_model_detail {
int pack_weights(ftc_model* m, Weights& w);                                                                    // pack.hip
int build_model_plan(ftc_model* m, int B, int H, int W, bool nchw, const PlanOptions& opt, ModelPlan* out);    // plan.hip
int build_decoder_plan(ftc_model* m, int rows, const PlanOptions& opt, ModelPlan* out);                        // plan.hip
}  // namespace ftc_model_detail
