// include/ftc_text.h: the text recognizer (models/transformer.py: Encoder, Decoder, TransformerPredictor) as a private launch sequence.
//
// Every nn.Linear is a 1x1 convolution over [1, rows, 1, C] run by the conv dispatcher (FTC_OP_CONV through ftc_plan_run), as
// build_decoder in model.hip runs SimpleDecoder; activations are fp32 in every mode and `precision` picks the GEMM arithmetic.  What
// the GEMM epilogues fuse: biases and ONE residual add (the attention / feed-forward output + its input); everything else is
// text_ops.hip, text_attention.hip and maskpredict_select.hip.  Per encoder block 9 launches, per decoder block 13:
//
//   [q | k] = (x + pos_q) . [Wq ; Wk]^T     one GEMM, N = 2E (self-attention: q and k inputs are the same tensor)
//   v       = x . Wv^T                       the value input carries no position table
//   a       = attention(q, k, v)             text_attention.hip
//   t       = a . Wo^T + x                   residual in the epilogue
//   x1      = LayerNorm(t)  (+ x1 + pos_q of the cross-attention as a second output in the decoder)
//   decoder only:  qc = (x1 + pos_q) . Wq^T;  a = attention(qc, Kc, Vc, key padding);  t = a . Wo^T + x1;  x2 = LayerNorm(t)
//   g       = x2 . [W1 ; Wg]^T + [b1 | bg]   one GEMM, N = 4E
//   h       = g[:, :2E] * silu(g[:, 2E:])
//   t       = h . W2^T + b2 + x2
//   x       = LayerNorm(t + x)               the block tail's second skip; second output x + pos_q of the next block
//
// The cross-attention keys and values do not depend on the pass: Kc_b = (enc + pos_k_b) . Wk_b^T per block and ONE GEMM for all
// blocks' values (N = blocks * E), once per call.  Rows of a batch never mix, and a row's bits do not depend on B: every GEMM runs the
// kernel choice of its B = 1 shape (no split-K, no 144-pixel tiles).
//
// include/ftc_text_compact.h: ftc_text_predict_compact runs pass p + 1 over the n rows still running after pass p.  A compact decoder
// pass is a plan with the WORKSPACE LAYOUT OF B AND THE ROW COUNT OF n, cached under (B, n) and built on first use; slot j of its n x 400
// activation rows stands for row map[j].  Four places see the map: the token-embedding row kernel (tokens of row map[j]), the
// cross-attention (K, V and padding of row map[j]), the selection (writes compact codes / scores: it simply runs on n x 400 positions)
// and the row update (reads slot j, writes tokens / ids / probs / done / traces of row map[j]).
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_text.h"
#include "../../include/ftc_text_compact.h"
#include "../../include/ftc_text_rows.h"
#include "../../include/ftc_text_attention16.h"

hipError_t ftc_text_attention_launch(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                                     float* out, int64_t ldo, int B, int heads, int Sq, int Sk, hipStream_t stream);
hipError_t ftc_text_attention_rows_launch(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                                          const int32_t* kv_row, int Bkv, float* out, int64_t ldo, int B, int heads, int Sq, int Sk, hipStream_t stream);
hipError_t ftc_text_attention16_launch(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                                       const int32_t* kv_row, int Bkv, float* out, int64_t ldo, int B, int heads, int Sq, int Sk, int operands,
                                       hipStream_t stream);
hipError_t ftc_text_rownorm_rows_launch(const float* a, const float* b, const float* pos_in, const float* gamma, const float* beta, const float* pos_out,
                                        const int64_t* tokens, const float* e0, const float* e1, const float* e2, const int32_t* tok_row, int tok_rows,
                                        float* out, float* out_pos, int64_t rows, int S, int E, hipStream_t stream);
hipError_t ftc_text_row_update_rows_launch(int64_t* tokens, const int64_t* codes, const float* scores, int B, int n, int pass, const int32_t* map,
                                           int32_t* done, int32_t* active, int64_t* ids, float* probs, int64_t* tr_tokens, int64_t* tr_codes,
                                           float* tr_probs, hipStream_t stream);
hipError_t ftc_text_row_map_launch(const int32_t* done, int B, int32_t* map, hipStream_t stream);
hipError_t ftc_text_rownorm_launch(const float* a, const float* b, const float* pos_in, const float* gamma, const float* beta, const float* pos_out,
                                   const int64_t* tokens, const float* e0, const float* e1, const float* e2, float* out, float* out_pos,
                                   int64_t rows, int S, int E, hipStream_t stream);
hipError_t ftc_text_swiglu_launch(const float* in, float* out, int64_t rows, int H, hipStream_t stream);
hipError_t ftc_text_pad_input_launch(const float* in, float* rows128, uint8_t* pad, int B, int L, int D, int S, hipStream_t stream);
hipError_t ftc_text_select_launch(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int64_t n,
                                  int64_t* codes, float* scores, float* top_p, int32_t* top_i, hipStream_t stream);
hipError_t ftc_text_row_update_launch(int64_t* tokens, const int64_t* codes, const float* scores, int B, int pass, int32_t* done, int32_t* active,
                                      int64_t* ids, float* probs, int64_t* tr_tokens, int64_t* tr_codes, float* tr_probs, hipStream_t stream);
hipError_t ftc_text_fill_tokens_launch(int64_t* tokens, int64_t n, int64_t value, hipStream_t stream);
void ftc_text_select_host_impl(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int64_t n, int64_t* codes,
                               float* scores, float* top_p, int32_t* top_i);

namespace {

constexpr int S = FTC_TEXT_LEN;
constexpr int KPAD = 128;                    // the 106-wide glyph vector padded to the K granularity of the GEMMs
constexpr int MOD[3] = {1091, 1093, 1097};
int64_t al(int64_t v) { return (v + 255) & ~int64_t(255); }

uint16_t bf16_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
uint16_t f16_rne(float f) {
    const _Float16 hv = (_Float16)(f > 65504.0f ? 65504.0f : f < -65504.0f ? -65504.0f : f);
    uint16_t u;
    std::memcpy(&u, &hv, 2);
    return u;
}
float f16_val(uint16_t u) {
    _Float16 hv;
    std::memcpy(&hv, &u, 2);
    return (float)hv;
}

struct Ctx {                                 // what a step needs at run time
    char* ws;
    const char* wt;
    hipStream_t s;
    const int64_t* tokens;
    float* logits[3];
};
using Step = std::function<int(const Ctx&)>;

struct Layout {
    int64_t xin, pad, enc, xp, qkv, att, t0, x1, g, hh, d, d2, kall, vall, logit[3], tokens, codes, scores, flags, total;
};

struct TextPlan {
    int B = 0;                               // workspace layout
    int n = 0;                               // rows of the decoder steps: B, or the slots of a compact pass (then enc and kv are empty)
    ftc_plan convs;
    std::vector<Step> enc, kv, dec;
    Layout L;
};

}  // namespace

struct ftc_text {
    ftc_text_dims d;
    int precision = FTC_F32;                 // FTC_F32 | FTC_BF16 | FTC_F16 | FTC_PRECISION_F16X3
    int attention = FTC_F32;                 // the attention's operands: FTC_F32 | FTC_F16 | FTC_BF16 (include/ftc_text_attention16.h)
    std::vector<uint8_t> blob;
    std::map<std::string, int64_t> off;
    std::mutex mu;
    std::map<std::pair<int, int>, std::shared_ptr<TextPlan>> plans;      // (B, 0): the whole call; (B, n): a compact decoder pass
};

namespace {

struct Packer {
    ftc_text* h;
    std::map<std::string, const ftc_tensor*> t;
    std::string err;

    const float* get(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = t.find(name);
        if (it == t.end()) { if (err.empty()) err = "missing tensor " + name; return nullptr; }
        const ftc_tensor* x = it->second;
        bool ok = x->dtype == FTC_F32 && x->ndim == (int)shape.size() && x->data;
        int i = 0;
        for (int64_t s : shape) { ok = ok && i < 4 && x->shape[i] == s; ++i; }
        if (!ok) { if (err.empty()) err = "tensor " + name + " has the wrong dtype or shape"; return nullptr; }
        return static_cast<const float*>(x->data);
    }
    uint8_t* add(const std::string& name, int64_t nbytes) {
        const int64_t o = (int64_t)h->blob.size();
        h->off[name] = o;
        h->blob.resize((size_t)al(o + nbytes), 0);
        return h->blob.data() + o;
    }
    void f32(const std::string& name, const float* v, int64_t n) {
        if (v) std::memcpy(add(name, n * 4), v, (size_t)n * 4);
    }
    // GEMM weight [sum rows][kpad] from row blocks of [rows_i][k] fp32 (K-major = the nn.Linear layout), in the operand format of the mode
    void w(const std::string& name, std::vector<std::pair<const float*, int64_t>> parts, int64_t k, int64_t kpad) {
        int64_t rows = 0;
        for (auto& p : parts) { if (!p.first) return; rows += p.second; }
        const int pr = h->precision;
        const int64_t n = rows * kpad;
        uint8_t* dst = add(name, n * (pr == FTC_BF16 || pr == FTC_F16 ? 2 : 4));
        int64_t r0 = 0;
        for (auto& p : parts) {
            for (int64_t r = 0; r < p.second; ++r) {
                const float* src = p.first + r * k;
                const int64_t o = (r0 + r) * kpad;
                if (pr == FTC_F32) {
                    std::memcpy(reinterpret_cast<float*>(dst) + o, src, (size_t)k * 4);
                } else if (pr == FTC_PRECISION_F16X3) {      // every 16-byte chunk of four fp32 weights: [hi x4 | lo x4] IEEE halves
                    uint16_t* d = reinterpret_cast<uint16_t*>(dst) + 2 * o;
                    for (int64_t i = 0; i < kpad; i += 4)
                        for (int e = 0; e < 4; ++e) {
                            const float x0 = i + e < k ? src[i + e] : 0.0f;
                            const float x = x0 > 65504.0f ? 65504.0f : x0 < -65504.0f ? -65504.0f : x0;      // the split's spec: clamp first, then hi, then lo
                            const uint16_t hi = f16_rne(x);
                            d[2 * i + e] = hi;
                            d[2 * i + 4 + e] = f16_rne(x - f16_val(hi));
                        }
                } else {
                    uint16_t* d = reinterpret_cast<uint16_t*>(dst) + o;
                    for (int64_t i = 0; i < k; ++i) d[i] = pr == FTC_BF16 ? bf16_rne(src[i]) : f16_rne(src[i]);
                }
            }
            r0 += p.second;
        }
    }
};

int pack(ftc_text* h, const ftc_tensor* tensors, int n) {
    Packer p{h, {}, {}};
    for (int i = 0; i < n; ++i)
        if (tensors[i].name) p.t[tensors[i].name] = &tensors[i];
    const ftc_text_dims& d = h->d;
    const int64_t E = d.embed_dim, D = d.enc_input_dim;
    auto attn = [&](const std::string& src, const std::string& dst, bool self) {
        const float *wq = p.get(src + ".q_proj.weight", {E, E}), *wk = p.get(src + ".k_proj.weight", {E, E}), *wv = p.get(src + ".v_proj.weight", {E, E}),
                    *wo = p.get(src + ".out_proj.weight", {E, E});
        const float *pq = p.get(src + ".pos_emb_q.encoding", {S, E}), *pk = p.get(src + ".pos_emb_k.encoding", {S, E});
        if (self) {
            p.w(dst + ".qk.w", {{wq, E}, {wk, E}}, E, E);
            p.w(dst + ".v.w", {{wv, E}}, E, E);
        } else {
            p.w(dst + ".q.w", {{wq, E}}, E, E);
            p.w(dst + ".k.w", {{wk, E}}, E, E);
            p.f32(dst + ".posk", pk, S * E);
        }
        p.w(dst + ".o.w", {{wo, E}}, E, E);
        p.f32(dst + ".posq", pq, S * E);
    };
    auto norm = [&](const std::string& src, const std::string& dst) {
        p.f32(dst + ".g", p.get(src + ".weight", {E}), E);
        p.f32(dst + ".b", p.get(src + ".bias", {E}), E);
    };
    auto ff = [&](const std::string& src, const std::string& dst) {
        const float *w1 = p.get(src + ".w1.weight", {2 * E, E}), *wg = p.get(src + ".wg.weight", {2 * E, E}), *w2 = p.get(src + ".w2.weight", {E, 2 * E});
        const float *b1 = p.get(src + ".w1.bias", {2 * E}), *bg = p.get(src + ".wg.bias", {2 * E}), *b2 = p.get(src + ".w2.bias", {E});
        p.w(dst + ".ff1.w", {{w1, 2 * E}, {wg, 2 * E}}, E, E);
        if (b1 && bg) {
            float* b = reinterpret_cast<float*>(p.add(dst + ".ff1.b", 4 * E * 4));
            std::memcpy(b, b1, (size_t)E * 8);
            std::memcpy(b + 2 * E, bg, (size_t)E * 8);
        }
        p.w(dst + ".ff2.w", {{w2, E}}, 2 * E, 2 * E);
        p.f32(dst + ".ff2.b", b2, E);
    };
    p.add("zero", std::max<int64_t>(d.dec_block_num * E, 4 * E) * 4);
    p.w("enc.embed.w", {{p.get("encoder.embed.weight", {E, D}), E}}, D, KPAD);
    p.f32("enc.pos", p.get("encoder.pos_emb.encoding", {S, E}), S * E);
    norm("encoder.norm", "enc.norm");
    for (int b = 0; b < d.enc_block_num; ++b) {
        const std::string s = "encoder.blocks." + std::to_string(b), t = "enc." + std::to_string(b);
        attn(s + ".mha", t + ".s", true);
        norm(s + ".norm1", t + ".n1"); norm(s + ".norm2", t + ".n2");
        ff(s + ".ff", t);
    }
    for (int i = 0; i < 3; ++i) p.f32("dec.emb" + std::to_string(i), p.get("decoder.embed." + std::to_string(i) + ".weight", {MOD[i], E}), MOD[i] * E);
    p.f32("dec.pos", p.get("decoder.pos_emb.encoding", {S, E}), S * E);
    norm("decoder.norm", "dec.norm");
    std::vector<std::pair<const float*, int64_t>> cv;
    for (int b = 0; b < d.dec_block_num; ++b) {
        const std::string s = "decoder.blocks." + std::to_string(b), t = "dec." + std::to_string(b);
        attn(s + ".self_attn", t + ".s", true);
        attn(s + ".cross_attn", t + ".c", false);
        cv.push_back({p.get(s + ".cross_attn.v_proj.weight", {E, E}), E});
        norm(s + ".norm1", t + ".n1"); norm(s + ".norm2", t + ".n2"); norm(s + ".norm3", t + ".n3");
        ff(s + ".ff", t);
    }
    p.w("dec.cv.w", cv, E, E);
    for (int i = 0; i < 3; ++i) {
        const std::string s = "decoder.out_layers." + std::to_string(i), t = "dec.out" + std::to_string(i);
        p.w(t + ".w", {{p.get(s + ".weight", {MOD[i], E}), MOD[i]}}, E, E);
        p.f32(t + ".b", p.get(s + ".bias", {MOD[i]}), MOD[i]);
    }
    // a GEMM tile that overhangs the last weight's rows (Cout = 1097 is no multiple of a tile) stays inside the blob: the widest tile of the
    // dispatcher is 192 weight rows (rounded up to 256 here) of at most K = 2E fp32 values
    p.add("tail", (int64_t)256 * 2 * E * 4);
    if (!p.err.empty()) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_create: " + p.err);
    return FTC_OK;
}

struct PlanBuilder {
    ftc_text* h;
    TextPlan* P;
    int B;                                   // the workspace layout is that of B rows
    int n;                                   // the steps run on n rows; n != B: a compact pass, slot j = row map[j]
    std::string err;
    int64_t R() const { return (int64_t)n * S; }
    bool compact() const { return n != B; }
    int64_t map_off() const { return P->L.flags + (int64_t)(FTC_TEXT_MAX_BATCH + FTC_TEXT_PASSES) * 4; }
    int64_t W(const std::string& name) {
        auto it = h->off.find(name);
        if (it == h->off.end()) { if (err.empty()) err = "internal: no packed tensor " + name; return 0; }
        return it->second;
    }
    // out[:, cout_off : cout_off + N] (row pitch ldo) = in[:, :K] (row pitch ldi) . w^T + bias (+ res); out_ws < 0: the logits pointer -(out_ws + 1)
    Step gemm(int64_t in, int K, int ldi, const std::string& w, const std::string& bias, int N, int64_t out_ws, int ldo, int cout_off, int64_t res = -1) {
        ftc_op o{};
        const int pr = h->precision;
        o.kind = FTC_OP_CONV;
        o.flags = (res >= 0 ? FTC_FLAG_RESIDUAL : 0) | (pr == FTC_PRECISION_F16X3 ? FTC_FLAG_SPLIT16 : 0);
        o.act = FTC_ACT_NONE;
        o.in_dtype = FTC_F32; o.out_dtype = FTC_F32; o.res_dtype = FTC_F32;
        o.w_dtype = pr == FTC_BF16 ? FTC_BF16 : pr == FTC_F16 ? FTC_F16 : FTC_F32;
        o.B = 1; o.H = S; o.W = 1; o.Ho = S; o.Wo = 1;          // the B = 1 shape decides the kernel; it is pinned for every batch
        o.Cin = K; o.Cin_total = ldi; o.Cout = N; o.Cout_total = ldo; o.cout_off = cout_off; o.ksize = 1; o.stride = 1;
        o.in = {FTC_BASE_WORKSPACE, 0, in};
        o.w = {FTC_BASE_WEIGHTS, 0, W(w)};
        o.bias = {FTC_BASE_WEIGHTS, 0, W(bias)};
        if (res >= 0) o.in2 = {FTC_BASE_WORKSPACE, 0, res};
        if (out_ws >= 0) o.out = {FTC_BASE_WORKSPACE, 0, out_ws};
        else o.out = {FTC_BASE_HEATMAP, 0, 0};
        // 400 rows: the default 128 x 64 tiles leave most of the MI355X's 256 CUs idle (the 256 below is that count), 64 x 64 tiles halve a workgroup's work.  The choice
        // (tile, staging, K step; never split-K or the 144-pixel tiles) is then written out in aux0 and used for every B: in the
        // 16-bit modes two tile configurations do not give the same bits (measured: tests/test_gpu_text.py, batch independence).
        if ((int64_t)((N + 127) / 128) * ((S + 63) / 64) < 256) {
            o.aux0 = conv_small_tile_choice();
            if (conv_validate(o)) o.aux0 = 0;
        }
        o.aux0 = conv_pinned_choice(o);
        o.H = o.Ho = (int)R();
        if (const char* why = conv_validate(o)) { if (err.empty()) err = std::string("GEMM ") + w + ": " + why; }
        const int idx = (int)P->convs.ops.size();
        P->convs.ops.push_back(o);
        const int head = out_ws < 0 ? (int)(-out_ws - 1) : -1;
        TextPlan* plan = P;
        return [plan, idx, head](const Ctx& c) {
            void* bases[FTC_NUM_BASES] = {nullptr, c.ws, const_cast<char*>(c.wt), nullptr, head >= 0 ? (void*)c.logits[head] : nullptr, nullptr, nullptr};
            return ftc_plan_run(&plan->convs, bases, c.s, idx, idx);
        };
    }
    static int hip(hipError_t e, const char* what) {
        return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_text: ") + what + ": " + hipGetErrorString(e));
    }
    // LayerNorm(a (+ b) (+ pos_in)) -> out, out + pos_out -> out_pos.  Weight-blob offsets < 0 = absent.
    Step norm(int64_t a, int64_t b, int64_t pos_in, const std::string& gb, int64_t out, int64_t pos_out, int64_t out_pos, bool tokens = false) {
        const int64_t g = gb.empty() ? -1 : W(gb + ".g"), be = gb.empty() ? -1 : W(gb + ".b");
        const int64_t e0 = tokens ? W("dec.emb0") : -1, e1 = tokens ? W("dec.emb1") : -1, e2 = tokens ? W("dec.emb2") : -1;
        const int64_t rows = R();
        const int E = h->d.embed_dim, B_ = B;
        const int64_t map = tokens && compact() ? map_off() : -1;
        return [=](const Ctx& c) {
            auto wsf = [&](int64_t o) { return o < 0 ? nullptr : reinterpret_cast<float*>(c.ws + o); };
            auto wtf = [&](int64_t o) { return o < 0 ? nullptr : reinterpret_cast<const float*>(c.wt + o); };
            return hip(ftc_text_rownorm_rows_launch(wsf(a), wsf(b), wtf(pos_in), wtf(g), wtf(be), wtf(pos_out), tokens ? c.tokens : nullptr, wtf(e0), wtf(e1),
                                                    wtf(e2), map < 0 ? nullptr : reinterpret_cast<const int32_t*>(c.ws + map), B_, wsf(out), wsf(out_pos),
                                                    rows, S, E, c.s), "row kernel");
        };
    }
    // cross: keys, values and padding are per-call state in the B-row layout (a compact pass reads them through the map); otherwise
    // q, k and v are this pass's own activations, slot by slot
    Step attention(int64_t q, int ldq, int64_t k, int ldk, int64_t v, int ldv, bool masked, int64_t out, bool cross = false) {
        const int B_ = B, n_ = n, heads = h->d.head_num, E = h->d.embed_dim;
        const int64_t pad = masked ? P->L.pad : -1;
        const int64_t map = cross && compact() ? map_off() : -1;
        if (const int operands = h->attention; operands != FTC_F32)          // the same launch on 16-bit operands (ftc_text_set_attention)
            return [=](const Ctx& c) {
                auto f = [&](int64_t o) { return reinterpret_cast<float*>(c.ws + o); };
                return hip(ftc_text_attention16_launch(f(q), ldq, f(k), ldk, f(v), ldv, pad < 0 ? nullptr : reinterpret_cast<const uint8_t*>(c.ws + pad),
                                                       map < 0 ? nullptr : reinterpret_cast<const int32_t*>(c.ws + map), map < 0 ? n_ : B_, f(out), E, n_, heads,
                                                       S, S, operands, c.s), "attention");
            };
        return [=](const Ctx& c) {
            auto f = [&](int64_t o) { return reinterpret_cast<float*>(c.ws + o); };
            return hip(ftc_text_attention_rows_launch(f(q), ldq, f(k), ldk, f(v), ldv, pad < 0 ? nullptr : reinterpret_cast<const uint8_t*>(c.ws + pad),
                                                      map < 0 ? nullptr : reinterpret_cast<const int32_t*>(c.ws + map), map < 0 ? n_ : B_, f(out), E, n_, heads,
                                                      S, S, c.s), "attention");
        };
    }
    Step swiglu(int64_t in, int64_t out) {
        const int64_t rows = R();
        const int H2 = 2 * h->d.embed_dim;
        return [=](const Ctx& c) {
            return hip(ftc_text_swiglu_launch(reinterpret_cast<const float*>(c.ws + in), reinterpret_cast<float*>(c.ws + out), rows, H2, c.s), "swiglu");
        };
    }

    int build() {
        const ftc_text_dims& d = h->d;
        const int E = d.embed_dim, NB = d.dec_block_num;
        const int64_t r = (int64_t)B * S;
        Layout& L = P->L;
        int64_t o = 0;
        auto take = [&](int64_t bytes) { const int64_t at = o; o += al(bytes); return at; };
        L.xin = take(r * KPAD * 4); L.pad = take(r);
        L.enc = take(r * E * 4); L.xp = take(r * E * 4); L.qkv = take(r * 3 * E * 4); L.att = take(r * E * 4); L.t0 = take(r * E * 4);
        L.x1 = take(r * E * 4); L.g = take(r * 4 * E * 4); L.hh = take(r * 2 * E * 4); L.d = take(r * E * 4); L.d2 = take(r * E * 4);
        L.kall = take(r * NB * E * 4); L.vall = take(r * NB * E * 4);
        for (int i = 0; i < 3; ++i) L.logit[i] = take(r * MOD[i] * 4);
        L.tokens = take(r * 8); L.codes = take(r * 8); L.scores = take(r * 4); L.flags = take((FTC_TEXT_MAX_BATCH + FTC_TEXT_PASSES + FTC_TEXT_MAX_BATCH) * 4);      // done, active, map
        L.total = o;
        auto ffn = [&](std::vector<Step>& st, const std::string& t, int64_t x) {          // x -> t0 = ff(x) + x
            st.push_back(gemm(x, E, E, t + ".ff1.w", t + ".ff1.b", 4 * E, L.g, 4 * E, 0));
            st.push_back(swiglu(L.g, L.hh));
            st.push_back(gemm(L.hh, 2 * E, 2 * E, t + ".ff2.w", t + ".ff2.b", E, L.t0, E, 0, x));
        };
        auto self_attn = [&](std::vector<Step>& st, const std::string& t, int64_t x, bool masked) {     // x, xp -> t0 = attn + x
            st.push_back(gemm(L.xp, E, E, t + ".s.qk.w", "zero", 2 * E, L.qkv, 3 * E, 0));
            st.push_back(gemm(x, E, E, t + ".s.v.w", "zero", E, L.qkv, 3 * E, 2 * E));
            st.push_back(attention(L.qkv, 3 * E, L.qkv + (int64_t)E * 4, 3 * E, L.qkv + (int64_t)2 * E * 4, 3 * E, masked, L.att));
            st.push_back(gemm(L.att, E, E, t + ".s.o.w", "zero", E, L.t0, E, 0, x));
        };
        // ---- encoder, and the cross-attention keys / values once per call (a compact pass finds both in the workspace)
        if (!compact()) {
            P->enc.push_back(gemm(L.xin, KPAD, KPAD, "enc.embed.w", "zero", E, L.t0, E, 0));
            P->enc.push_back(norm(L.t0, -1, W("enc.pos"), "enc.norm", L.enc, d.enc_block_num ? W("enc.0.s.posq") : -1, d.enc_block_num ? L.xp : -1));
            for (int b = 0; b < d.enc_block_num; ++b) {
                const std::string t = "enc." + std::to_string(b);
                self_attn(P->enc, t, L.enc, true);
                P->enc.push_back(norm(L.t0, -1, -1, t + ".n1", L.x1, -1, -1));
                ffn(P->enc, t, L.x1);
                const bool last = b + 1 == d.enc_block_num;
                P->enc.push_back(norm(L.t0, L.enc, -1, t + ".n2", L.enc, last ? -1 : W("enc." + std::to_string(b + 1) + ".s.posq"), last ? -1 : L.xp));
            }
            // ---- cross-attention keys / values
            for (int b = 0; b < NB; ++b) {
                const std::string t = "dec." + std::to_string(b);
                P->kv.push_back(norm(L.enc, -1, -1, "", -1, W(t + ".c.posk"), L.xp));
                P->kv.push_back(gemm(L.xp, E, E, t + ".c.k.w", "zero", E, L.kall, NB * E, b * E));
            }
            if (NB) P->kv.push_back(gemm(L.enc, E, E, "dec.cv.w", "zero", NB * E, L.vall, NB * E, 0));
        }
        // ---- one decoder pass
        P->dec.push_back(norm(-1, -1, W("dec.pos"), "dec.norm", L.d, NB ? W("dec.0.s.posq") : -1, NB ? L.xp : -1, true));
        for (int b = 0; b < NB; ++b) {
            const std::string t = "dec." + std::to_string(b);
            self_attn(P->dec, t, L.d, false);
            P->dec.push_back(norm(L.t0, -1, -1, t + ".n1", L.x1, W(t + ".c.posq"), L.xp));
            P->dec.push_back(gemm(L.xp, E, E, t + ".c.q.w", "zero", E, L.qkv, 3 * E, 0));
            P->dec.push_back(attention(L.qkv, 3 * E, L.kall + (int64_t)b * E * 4, NB * E, L.vall + (int64_t)b * E * 4, NB * E, true, L.att, true));
            P->dec.push_back(gemm(L.att, E, E, t + ".c.o.w", "zero", E, L.t0, E, 0, L.x1));
            P->dec.push_back(norm(L.t0, -1, -1, t + ".n2", L.d2, -1, -1));
            ffn(P->dec, t, L.d2);
            const bool last = b + 1 == NB;
            P->dec.push_back(norm(L.t0, L.d, -1, t + ".n3", L.d, last ? -1 : W("dec." + std::to_string(b + 1) + ".s.posq"), last ? -1 : L.xp));
        }
        for (int i = 0; i < 3; ++i) {
            const std::string t = "dec.out" + std::to_string(i);
            P->dec.push_back(gemm(L.d, E, E, t + ".w", t + ".b", MOD[i], -(i + 1), MOD[i], 0));
        }
        if (!err.empty()) return ftc_set_error(FTC_ERR_INVALID, "ftc_text plan: " + err);
        P->convs.workspace_bytes = L.total;
        P->convs.weights_bytes = (int64_t)h->blob.size();
        ftc_plan* checked = nullptr;
        int rc = ftc_plan_create(P->convs.ops.data(), (int)P->convs.ops.size(), L.total, P->convs.weights_bytes, &checked);
        if (rc != FTC_OK) return rc;
        ftc_plan_destroy(checked);
        return FTC_OK;
    }
};

// n = 0: the plan of a whole call with B rows; 1 <= n < B: the decoder pass over n compact slots in the layout of B
int get_plan(ftc_text* h, int B, std::shared_ptr<TextPlan>* out, int n = 0) {
    if (!h) return ftc_set_error(FTC_ERR_INVALID, "ftc_text: null handle");
    if (B < 1 || B > FTC_TEXT_MAX_BATCH) return ftc_set_error(FTC_ERR_INVALID, "ftc_text: B must be in 1.." + std::to_string(FTC_TEXT_MAX_BATCH) + " (split the batch)");
    if (n < 0 || n >= B) n = 0;
    std::lock_guard<std::mutex> lk(h->mu);
    const std::pair<int, int> key(B, n);
    auto it = h->plans.find(key);
    if (it == h->plans.end()) {
        std::shared_ptr<TextPlan> p(new (std::nothrow) TextPlan());
        if (!p) return ftc_set_error(FTC_ERR_NOMEM, "ftc_text: out of host memory");
        p->B = B;
        p->n = n ? n : B;
        PlanBuilder pb{h, p.get(), B, p->n, {}};
        const int rc = pb.build();
        if (rc != FTC_OK) return rc;
        it = h->plans.emplace(key, std::move(p)).first;
    }
    *out = it->second;
    return FTC_OK;
}

int run(const std::vector<Step>& steps, const Ctx& c) {
    for (const Step& s : steps) {
        const int rc = s(c);
        if (rc != FTC_OK) return rc;
    }
    return FTC_OK;
}

int encode(ftc_text* h, TextPlan& P, const Ctx& c, const float* enc_input, int B, int L, float* enc_out) {
    if (L < 1 || L > S) return ftc_set_error(FTC_ERR_INVALID, "ftc_text: L must be in 1.." + std::to_string(S));
    int rc = PlanBuilder::hip(ftc_text_pad_input_launch(enc_input, reinterpret_cast<float*>(c.ws + P.L.xin), reinterpret_cast<uint8_t*>(c.ws + P.L.pad), B, L,
                                                        h->d.enc_input_dim, S, c.s), "input padding");
    if (rc == FTC_OK) rc = run(P.enc, c);
    if (rc == FTC_OK) rc = run(P.kv, c);
    if (rc == FTC_OK && enc_out)
        rc = PlanBuilder::hip(hipMemcpyAsync(enc_out, c.ws + P.L.enc, (size_t)B * S * h->d.embed_dim * 4, hipMemcpyDeviceToDevice, c.s), "encoder output copy");
    return rc;
}

}  // namespace

extern "C" {

int ftc_text_abi_version(void) { return FTC_TEXT_ABI_VERSION; }

int ftc_text_create(const ftc_tensor* tensors, int n_tensors, const ftc_text_dims* dims, int precision, ftc_text** out) {
    if (!tensors || n_tensors <= 0 || !dims || !out) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_create: null/empty arguments");
    if (precision != FTC_F32 && precision != FTC_BF16 && precision != FTC_F16 && precision != FTC_PRECISION_F16X3)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_create: precision must be FTC_F32, FTC_BF16, FTC_F16 or FTC_PRECISION_F16X3");
    const ftc_text_dims& d = *dims;
    if (d.head_num < 1 || d.head_num > 16 || d.embed_dim != 64 * d.head_num)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_create: the attention kernel needs heads of width 64: embed_dim == 64 * head_num, head_num <= 16 (got embed_dim " +
                                                  std::to_string(d.embed_dim) + ", head_num " + std::to_string(d.head_num) + ")");
    if (d.max_enc_seq_len != S || d.max_dec_seq_len != S)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_create: max_enc_seq_len and max_dec_seq_len must be " + std::to_string(S));
    if (d.enc_input_dim < 1 || d.enc_input_dim > KPAD) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_create: enc_input_dim must be in 1..128");
    if (d.enc_block_num < 0 || d.enc_block_num > 64 || d.dec_block_num < 0 || d.dec_block_num > 64 || d.reserved != 0)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_create: block counts must be in 0..64 and reserved 0");
    std::unique_ptr<ftc_text> h(new (std::nothrow) ftc_text());
    if (!h) return ftc_set_error(FTC_ERR_NOMEM, "ftc_text_create: out of host memory");
    h->d = d;
    h->precision = precision;
    const int rc = pack(h.get(), tensors, n_tensors);
    if (rc != FTC_OK) return rc;
    *out = h.release();
    return FTC_OK;
}

void ftc_text_destroy(ftc_text* h) { delete h; }
int64_t ftc_text_weights_bytes(const ftc_text* h) { return h ? (int64_t)h->blob.size() : -1; }
const void* ftc_text_weights_host(const ftc_text* h) { return h ? h->blob.data() : nullptr; }

int64_t ftc_text_workspace_bytes(ftc_text* h, int B) {
    std::shared_ptr<TextPlan> p;
    if (get_plan(h, B, &p) != FTC_OK) return -1;
    return p->L.total;
}

int ftc_text_launch_count(ftc_text* h, int which) {
    std::shared_ptr<TextPlan> p;
    if (get_plan(h, 1, &p) != FTC_OK) return -1;
    switch (which) {
    case 0: return (int)p->enc.size() + 1;
    case 1: return (int)p->kv.size();
    case 2: return (int)p->dec.size();
    case 3: return 2;
    default: ftc_set_error(FTC_ERR_INVALID, "ftc_text_launch_count: which must be 0..3"); return -1;
    }
}

int ftc_text_encode(ftc_text* h, const void* weights_dev, const float* enc_input, int B, int L, float* enc_out, void* workspace, void* stream) {
    if (!weights_dev || !enc_input || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_encode: null pointer argument");
    std::shared_ptr<TextPlan> p;
    const int rc = get_plan(h, B, &p);
    if (rc != FTC_OK) return rc;
    const Ctx c{static_cast<char*>(workspace), static_cast<const char*>(weights_dev), static_cast<hipStream_t>(stream), nullptr, {nullptr, nullptr, nullptr}};
    return encode(h, *p, c, enc_input, B, L, enc_out);
}

int ftc_text_decode_step(ftc_text* h, const void* weights_dev, const int64_t* tokens, int B, float* logits0, float* logits1, float* logits2,
                         void* workspace, void* stream) {
    if (!weights_dev || !tokens || !logits0 || !logits1 || !logits2 || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_decode_step: null pointer argument");
    std::shared_ptr<TextPlan> p;
    const int rc = get_plan(h, B, &p);
    if (rc != FTC_OK) return rc;
    const Ctx c{static_cast<char*>(workspace), static_cast<const char*>(weights_dev), static_cast<hipStream_t>(stream), tokens, {logits0, logits1, logits2}};
    return run(p->dec, c);
}

int ftc_text_predict(ftc_text* h, const void* weights_dev, const float* enc_input, int B, int L, int64_t* ids, float* probs, int64_t* trace_tokens,
                     int64_t* trace_codes, float* trace_probs, int flags, int* passes_run, void* workspace, void* stream) {
    if (!weights_dev || !enc_input || !ids || !probs || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_predict: null pointer argument");
    std::shared_ptr<TextPlan> p;
    int rc = get_plan(h, B, &p);
    if (rc != FTC_OK) return rc;
    char* ws = static_cast<char*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Layout& L_ = p->L;
    int64_t* tokens = reinterpret_cast<int64_t*>(ws + L_.tokens);
    int64_t* codes = reinterpret_cast<int64_t*>(ws + L_.codes);
    float* scores = reinterpret_cast<float*>(ws + L_.scores);
    int32_t* done = reinterpret_cast<int32_t*>(ws + L_.flags);
    int32_t* active = done + FTC_TEXT_MAX_BATCH;
    float* lg[3];
    for (int i = 0; i < 3; ++i) lg[i] = reinterpret_cast<float*>(ws + L_.logit[i]);
    const Ctx c{ws, static_cast<const char*>(weights_dev), s, tokens, {lg[0], lg[1], lg[2]}};
    rc = encode(h, *p, c, enc_input, B, L, nullptr);
    if (rc != FTC_OK) return rc;
    const int64_t n = (int64_t)B * S;
    rc = PlanBuilder::hip(ftc_text_fill_tokens_launch(tokens, n, FTC_TEXT_MASK_TOKEN, s), "token fill");
    if (rc == FTC_OK) rc = PlanBuilder::hip(hipMemsetAsync(done, 0, (FTC_TEXT_MAX_BATCH + FTC_TEXT_PASSES) * 4, s), "flag reset");
    int pass = 0;
    for (; rc == FTC_OK && pass < FTC_TEXT_PASSES; ++pass) {
        rc = run(p->dec, c);
        if (rc == FTC_OK) rc = PlanBuilder::hip(ftc_text_select_launch(lg[0], lg[1], lg[2], MOD[0], MOD[1], MOD[2], n, codes, scores, nullptr, nullptr, s), "selection");
        if (rc == FTC_OK)
            rc = PlanBuilder::hip(ftc_text_row_update_launch(tokens, codes, scores, B, pass, done, active, ids, probs, trace_tokens, trace_codes, trace_probs, s),
                                  "row update");
        if (rc == FTC_OK && !(flags & FTC_TEXT_NO_READBACK) && pass + 1 < FTC_TEXT_PASSES) {
            int32_t still = 0;
            rc = PlanBuilder::hip(hipMemcpyAsync(&still, active + pass, 4, hipMemcpyDeviceToHost, s), "active-row read");
            if (rc == FTC_OK) rc = PlanBuilder::hip(hipStreamSynchronize(s), "active-row read");
            if (rc == FTC_OK && still == 0) { ++pass; break; }
        }
    }
    if (passes_run) *passes_run = pass;
    return rc;
}

int ftc_text_compact_abi_version(void) { return FTC_TEXT_COMPACT_ABI_VERSION; }

int ftc_text_predict_compact(ftc_text* h, const void* weights_dev, const float* enc_input, int B, int L, int64_t* ids, float* probs, int64_t* trace_tokens,
                             int64_t* trace_codes, float* trace_probs, int flags, int* passes_run, int* rows_run, void* workspace, void* stream) {
    if (!weights_dev || !enc_input || !ids || !probs || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_predict_compact: null pointer argument");
    if (flags & FTC_TEXT_NO_READBACK)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_predict_compact: FTC_TEXT_NO_READBACK is refused: the number of rows of the next pass is read back after "
                                              "every pass (ftc_text_predict is the loop that runs without a host read)");
    std::shared_ptr<TextPlan> p, cp;
    int rc = get_plan(h, B, &p);
    if (rc != FTC_OK) return rc;
    char* ws = static_cast<char*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Layout& L_ = p->L;
    int64_t* tokens = reinterpret_cast<int64_t*>(ws + L_.tokens);
    int64_t* codes = reinterpret_cast<int64_t*>(ws + L_.codes);
    float* scores = reinterpret_cast<float*>(ws + L_.scores);
    int32_t* done = reinterpret_cast<int32_t*>(ws + L_.flags);
    int32_t* active = done + FTC_TEXT_MAX_BATCH;
    int32_t* map = active + FTC_TEXT_PASSES;
    float* lg[3];
    for (int i = 0; i < 3; ++i) lg[i] = reinterpret_cast<float*>(ws + L_.logit[i]);
    const Ctx c{ws, static_cast<const char*>(weights_dev), s, tokens, {lg[0], lg[1], lg[2]}};
    if (rows_run) std::memset(rows_run, 0, sizeof(int) * FTC_TEXT_PASSES);
    rc = encode(h, *p, c, enc_input, B, L, nullptr);
    if (rc != FTC_OK) return rc;
    rc = PlanBuilder::hip(ftc_text_fill_tokens_launch(tokens, (int64_t)B * S, FTC_TEXT_MASK_TOKEN, s), "token fill");
    if (rc == FTC_OK) rc = PlanBuilder::hip(hipMemsetAsync(done, 0, (FTC_TEXT_MAX_BATCH + FTC_TEXT_PASSES) * 4, s), "flag reset");
    int pass = 0, n = B;                     // n rows run in this pass; n < B: slot j is row map[j]
    for (; rc == FTC_OK && pass < FTC_TEXT_PASSES; ++pass) {
        rc = run(n == B ? p->dec : cp->dec, c);
        if (rc == FTC_OK)
            rc = PlanBuilder::hip(ftc_text_select_launch(lg[0], lg[1], lg[2], MOD[0], MOD[1], MOD[2], (int64_t)n * S, codes, scores, nullptr, nullptr, s), "selection");
        if (rc == FTC_OK)
            rc = PlanBuilder::hip(ftc_text_row_update_rows_launch(tokens, codes, scores, B, n, pass, n == B ? nullptr : map, done, active, ids, probs, trace_tokens,
                                                                  trace_codes, trace_probs, s), "row update");
        if (rc == FTC_OK && rows_run) rows_run[pass] = n;
        if (rc == FTC_OK && pass + 1 < FTC_TEXT_PASSES) {
            int32_t still = 0;
            rc = PlanBuilder::hip(ftc_text_row_map_launch(done, B, map, s), "row map");
            if (rc == FTC_OK) rc = PlanBuilder::hip(hipMemcpyAsync(&still, active + pass, 4, hipMemcpyDeviceToHost, s), "active-row read");
            if (rc == FTC_OK) rc = PlanBuilder::hip(hipStreamSynchronize(s), "active-row read");
            if (rc == FTC_OK && still == 0) { ++pass; break; }
            if (rc == FTC_OK && (still < 0 || still > n)) rc = ftc_set_error(FTC_ERR_HIP, "ftc_text_predict_compact: the active-row count grew between passes");
            if (rc == FTC_OK && still != n) {
                n = still;
                rc = get_plan(h, B, &cp, n);
            }
        }
    }
    if (passes_run) *passes_run = pass;
    return rc;
}

int ftc_text_set_attention(ftc_text* h, int operands) {
    if (!h) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_set_attention: null handle");
    if (operands != FTC_F32 && operands != FTC_F16 && operands != FTC_BF16)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_set_attention: operands must be FTC_F32, FTC_F16 or FTC_BF16");
    std::lock_guard<std::mutex> lk(h->mu);
    h->attention = operands;
    h->plans.clear();                        // a call in flight keeps its plan alive (shared_ptr); the next one builds with the new choice
    return FTC_OK;
}

int ftc_text_get_attention(const ftc_text* h) {
    if (!h) { ftc_set_error(FTC_ERR_INVALID, "ftc_text_get_attention: null handle"); return -1; }
    return h->attention;
}

static bool ld_ok(int64_t ld, int heads) { return ld >= 64 * (int64_t)heads && ld % 4 == 0; }

int ftc_text_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad, float* out,
                       int64_t ldo, int B, int heads, int Sq, int Sk, void* stream) {
    if (!q || !k || !v || !out) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention: null pointer argument");
    if (B < 1 || B > 65535 || heads < 1 || heads > 1024 || Sq < 1 || Sq > S || Sk < 1 || Sk > S)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention: B, heads >= 1 and 1 <= Sq, Sk <= " + std::to_string(S));
    if (!ld_ok(ldq, heads) || !ld_ok(ldk, heads) || !ld_ok(ldv, heads) || !ld_ok(ldo, heads) || ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention: row pitches must be multiples of 4 floats and at least 64 * heads, q / k / v 16-byte aligned");
    return PlanBuilder::hip(ftc_text_attention_launch(q, ldq, k, ldk, v, ldv, key_pad, out, ldo, B, heads, Sq, Sk, static_cast<hipStream_t>(stream)), "attention");
}

int ftc_text_attention_rows(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                            const int32_t* kv_row, int Bkv, float* out, int64_t ldo, int B, int heads, int Sq, int Sk, void* stream) {
    if (!q || !k || !v || !out) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_rows: null pointer argument");
    if (B < 1 || B > 65535 || Bkv < 1 || Bkv > 65535 || heads < 1 || heads > 1024 || Sq < 1 || Sq > S || Sk < 1 || Sk > S)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_rows: B, Bkv, heads >= 1 and 1 <= Sq, Sk <= " + std::to_string(S));
    if (!kv_row && Bkv != B) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_rows: a NULL kv_row is the identity and needs Bkv == B");
    if (!ld_ok(ldq, heads) || !ld_ok(ldk, heads) || !ld_ok(ldv, heads) || !ld_ok(ldo, heads) || ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 || (uintptr_t)kv_row % 4)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_rows: row pitches must be multiples of 4 floats and at least 64 * heads, q / k / v 16-byte aligned");
    // the entries of kv_row are device data: the kernel checks each against Bkv before it forms an address
    return PlanBuilder::hip(ftc_text_attention_rows_launch(q, ldq, k, ldk, v, ldv, key_pad, kv_row, Bkv, out, ldo, B, heads, Sq, Sk, static_cast<hipStream_t>(stream)),
                            "attention");
}

int ftc_text_rownorm(const float* a, const float* b, const float* pos_in, const float* gamma, const float* beta, const float* pos_out,
                     const int64_t* tokens, const float* e0, const float* e1, const float* e2, float* out, float* out_pos, int64_t rows, int S_, int E,
                     void* stream) {
    if ((!a && !tokens) || (tokens && (!e0 || !e1 || !e2)) || (!out && !out_pos) || (out_pos && !pos_out) || (gamma && !beta))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_rownorm: inconsistent pointer arguments");
    if (rows < 0 || S_ < 1 || E < 64 || E > 1024 || E % 64) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_rownorm: E must be a multiple of 64 in 64..1024, S >= 1");
    return PlanBuilder::hip(ftc_text_rownorm_launch(a, b, pos_in, gamma, beta, pos_out, tokens, e0, e1, e2, out, out_pos, rows, S_, E,
                                                    static_cast<hipStream_t>(stream)), "row kernel");
}

int ftc_text_swiglu(const float* in, float* out, int64_t rows, int H, void* stream) {
    if (!in || !out || rows < 0 || H < 4 || H % 4 || ((uintptr_t)in | (uintptr_t)out) % 16)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_swiglu: H must be a positive multiple of 4, pointers 16-byte aligned");
    return PlanBuilder::hip(ftc_text_swiglu_launch(in, out, rows, H, static_cast<hipStream_t>(stream)), "swiglu");
}

int ftc_text_select(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int64_t n, int64_t* codes, float* scores,
                    float* top_p, int32_t* top_i, void* stream) {
    if (!l0 || !l1 || !l2 || !codes || !scores || (top_p != nullptr) != (top_i != nullptr)) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_select: null pointer argument");
    if (n < 0 || n > (int64_t(1) << 30) || ld0 < MOD[0] || ld1 < MOD[1] || ld2 < MOD[2]) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_select: bad n or row pitch");
    return PlanBuilder::hip(ftc_text_select_launch(l0, l1, l2, ld0, ld1, ld2, n, codes, scores, top_p, top_i, static_cast<hipStream_t>(stream)), "selection");
}

int ftc_text_select_host(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int64_t n, int64_t* codes, float* scores,
                         float* top_p, int32_t* top_i) {
    if (!l0 || !l1 || !l2 || !codes || !scores || (top_p != nullptr) != (top_i != nullptr)) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_select_host: null pointer argument");
    if (n < 0 || ld0 < MOD[0] || ld1 < MOD[1] || ld2 < MOD[2]) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_select_host: bad n or row pitch");
    ftc_text_select_host_impl(l0, l1, l2, ld0, ld1, ld2, n, codes, scores, top_p, top_i);
    return FTC_OK;
}

int ftc_text_row_update(int64_t* tokens, const int64_t* codes, const float* scores, int B, int pass, int32_t* done, int32_t* active, int64_t* ids,
                        float* probs, int64_t* trace_tokens, int64_t* trace_codes, float* trace_probs, void* stream) {
    if (!tokens || !codes || !scores || !done || !active || !ids || !probs) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_row_update: null pointer argument");
    if (B < 1 || B > 65535 || pass < 0 || pass >= FTC_TEXT_PASSES) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_row_update: bad B or pass");
    return PlanBuilder::hip(ftc_text_row_update_launch(tokens, codes, scores, B, pass, done, active, ids, probs, trace_tokens, trace_codes, trace_probs,
                                                       static_cast<hipStream_t>(stream)), "row update");
}

int ftc_text_rows_abi_version(void) { return FTC_TEXT_ROWS_ABI_VERSION; }

int ftc_text_rownorm_rows(const float* a, const float* b, const float* pos_in, const float* gamma, const float* beta, const float* pos_out,
                          const int64_t* tokens, const float* e0, const float* e1, const float* e2, const int32_t* tok_row, int tok_rows, float* out,
                          float* out_pos, int64_t rows, int S_, int E, void* stream) {
    if ((!a && !tokens) || (tokens && (!e0 || !e1 || !e2)) || (!out && !out_pos) || (out_pos && !pos_out) || (gamma && !beta))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_rownorm_rows: inconsistent pointer arguments");
    if (rows < 0 || S_ < 1 || E < 64 || E > 1024 || E % 64) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_rownorm_rows: E must be a multiple of 64 in 64..1024, S >= 1");
    if (tok_row && (!tokens || tok_rows < 1 || (uintptr_t)tok_row % 4))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_rownorm_rows: tok_row needs tokens and tok_rows >= 1");
    // the entries of tok_row are device data: the kernel checks each against tok_rows before it forms an address
    return PlanBuilder::hip(ftc_text_rownorm_rows_launch(a, b, pos_in, gamma, beta, pos_out, tokens, e0, e1, e2, tok_row, tok_rows, out, out_pos, rows, S_, E,
                                                         static_cast<hipStream_t>(stream)), "row kernel");
}

int ftc_text_pad_input(const float* in, float* rows128, uint8_t* pad, int B, int L, int D, int S_, void* stream) {
    if (!in || !rows128 || !pad) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_pad_input: null pointer argument");
    if (D < 1 || D > KPAD || L < 1 || L > S_ || B < 1) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_pad_input: 1 <= D <= 128, 1 <= L <= S and B >= 1");
    return PlanBuilder::hip(ftc_text_pad_input_launch(in, rows128, pad, B, L, D, S_, static_cast<hipStream_t>(stream)), "input padding");
}

int ftc_text_plan_ops(ftc_text* h, int B, int n, ftc_op* out, int cap) {
    if (n < 0 || (n && n >= B) || cap < 0 || (cap && !out)) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_plan_ops: 0 <= n < B, cap >= 0, out needed when cap > 0");
    std::shared_ptr<TextPlan> p;
    const int rc = get_plan(h, B, &p, n);
    if (rc != FTC_OK) return rc;
    int count = 0;
    for (const ftc_op& o : p->convs.ops) {      // pushed in the order the steps are built: encoder, key / value, decoder
        if (o.kind != FTC_OP_CONV) continue;
        if (count < cap) out[count] = o;
        ++count;
    }
    return count;
}

}  // extern "C"
