// Weight packing behind ftc_create (once per checkpoint): eval-mode BatchNorm folded into the preceding convolution in float64, K-major
// [Cout][kh*kw][Cin] re-layout, conversion to the MFMA compute type, one blob (model_net.h: Blob).
// Host-only code: no kernels here.  Compiled with -ffp-contract=off so the float64 folding is the plain multiply / subtract sequence
// (no fused rounding differences between builds).
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>

#include "model_net.h"

namespace ftc_model_detail {

const TensorView* Weights::get(const std::string& k, std::initializer_list<int64_t> shape) {
    auto it = t.find(k);
    if (it == t.end()) { if (missing.empty()) missing = "missing tensor '" + k + "'"; return nullptr; }
    if (it->second.shape != std::vector<int64_t>(shape)) {
        if (missing.empty()) {
            missing = "tensor '" + k + "' has shape [";
            for (auto s : it->second.shape) missing += std::to_string(s) + ",";
            missing += "], expected [";
            for (auto s : shape) missing += std::to_string(s) + ",";
            missing += "]";
        }
        return nullptr;
    }
    return &it->second;
}

namespace {

inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);      // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

inline float f16_to_f32(uint16_t u) {
    _Float16 h;
    std::memcpy(&h, &u, 2);
    return (float)h;
}

inline uint16_t f32_to_f16_rne(float f) {           // IEEE half, round-to-nearest-even, saturating like the device stores
    if (f > 65504.0f) f = 65504.0f;
    if (f < -65504.0f) f = -65504.0f;
    const _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}

// The fold / re-layout / conversion loops below touch every one of the 262 M weights in float64: on one thread ftc_create took 5-9 s.
// par_for splits an index range over a few threads when it is large (results do not depend on the split: every index is independent).
template <typename F>
void par_for(int64_t n, int64_t grain, F&& f) {          // f(begin, end); begin is a multiple of `grain`
    const int64_t chunks = (n + grain - 1) / grain;
    int nt = (int)std::min<int64_t>(std::min<unsigned>(8, std::max(1u, std::thread::hardware_concurrency())), chunks);
    if (n < (int64_t)1 << 18 || nt <= 1) { f(0, n); return; }
    std::vector<std::thread> th;
    const int64_t per = (chunks + nt - 1) / nt * grain;
    for (int t = 0; t < nt; ++t) {
        const int64_t b = t * per, e = std::min(n, b + per);
        if (b < e) th.emplace_back([&f, b, e] { f(b, e); });
    }
    for (auto& x : th) x.join();
}

}  // namespace

uint8_t* Blob::add(const std::string& name, int64_t nbytes) {
    const int64_t off = (int64_t)bytes.size();
    table[name] = off;
    bytes.resize((size_t)align_up(off + nbytes), 0);
    return bytes.data() + off;
}
void Blob::add_f32(const std::string& name, const double* v, int64_t n) {
    float* d = reinterpret_cast<float*>(add(name, n * 4));
    par_for(n, 1024, [&](int64_t b, int64_t e) { for (int64_t i = b; i < e; ++i) d[i] = (float)v[i]; });
}
void Blob::add_f32(const std::string& name, const float* v, int64_t n) { std::memcpy(add(name, n * 4), v, (size_t)n * 4); }
void Blob::add_compute(const std::string& name, const double* v, int64_t n, int dt) {
    if (dt == FTC_F32) { add_f32(name, v, n); return; }
    if (dt == FTC_PRECISION_F16X3) {                    // fp16x3: every 16-byte chunk of four fp32 weights becomes [hi x4 | lo x4] IEEE halves
        uint16_t* d = reinterpret_cast<uint16_t*>(add(name, n * 4));
        std::atomic<bool> beyond{false};
        par_for(n, 1024, [&](int64_t b, int64_t en) {
            bool bad = false;
            for (int64_t i = b; i + 3 < en; i += 4)
                for (int e = 0; e < 4; ++e) {
                    const float x = (float)v[i + e];
                    bad |= !(std::fabs(x) <= 65504.0f);              // NaN included
                    const float xs = x > 65504.0f ? 65504.0f : x < -65504.0f ? -65504.0f : x;      // the split's spec: clamp, then hi, then lo of the clamped value
                    const uint16_t h = f32_to_f16_rne(xs);
                    d[2 * i + e] = h;
                    d[2 * i + 4 + e] = f32_to_f16_rne(xs - f16_to_f32(h));
                }
            if (bad) beyond = true;
        });
        if (beyond && out_of_range.empty()) out_of_range = name;
        return;
    }
    uint16_t* d = reinterpret_cast<uint16_t*>(add(name, n * 2));
    if (dt == FTC_BF16) par_for(n, 1024, [&](int64_t b, int64_t e) { for (int64_t i = b; i < e; ++i) d[i] = f32_to_bf16_rne((float)v[i]); });
    else par_for(n, 1024, [&](int64_t b, int64_t e) { for (int64_t i = b; i < e; ++i) d[i] = f32_to_f16_rne((float)v[i]); });
}

namespace {

struct BnAffine { std::vector<double> s, t; };     // y = x*s + t  (eval-mode BatchNorm)

bool bn_affine(Weights& w, const std::string& p, int c, double eps, BnAffine* out) {
    const TensorView *g = w.get(p + ".weight", {c}), *b = w.get(p + ".bias", {c}), *m = w.get(p + ".running_mean", {c}),
                     *v = w.get(p + ".running_var", {c});
    if (!g || !b || !m || !v) return false;
    out->s.resize(c);
    out->t.resize(c);
    for (int i = 0; i < c; ++i) {
        const double s = (double)g->data[i] / std::sqrt((double)v->data[i] + eps);
        out->s[i] = s;
        out->t[i] = (double)b->data[i] - (double)m->data[i] * s;
    }
    return true;
}

// conv weight [O,I,kh,kw] followed by an eval BN -> (W*s in OIHW order, float64; bias float64)
bool fold(Weights& w, const std::string& conv_key, const std::string& bn_prefix, double eps, int O, int I, int k, std::vector<double>* wf,
          std::vector<double>* bias) {
    const TensorView* cw = w.get(conv_key, {O, I, k, k});
    BnAffine a;
    if (!cw || !bn_affine(w, bn_prefix, O, eps, &a)) return false;
    const int64_t per = (int64_t)I * k * k;
    wf->resize((size_t)O * per);
    par_for((int64_t)O * per, per, [&](int64_t b, int64_t e) {
        for (int64_t o = b / per; o * per < e; ++o) {
            const double s = a.s[o];
            const float* src = cw->data + o * per;
            double* dst = wf->data() + o * per;
            for (int64_t i = 0; i < per; ++i) dst[i] = (double)src[i] * s;
        }
    });
    *bias = a.t;
    return true;
}

// [O,I,kh,kw] -> [O, kh*kw, I]
std::vector<double> kmajor(const std::vector<double>& w, int O, int I, int k) {
    std::vector<double> out(w.size());
    const int kk = k * k;
    const int64_t per = (int64_t)I * kk;
    par_for((int64_t)O * per, per, [&](int64_t b, int64_t e) {
        for (int64_t o = b / per; o * per < e; ++o)
            for (int i = 0; i < I; ++i)
                for (int t = 0; t < kk; ++t) out[((size_t)o * kk + t) * I + i] = w[((size_t)o * I + i) * kk + t];
    });
    return out;
}

// Bias table of a 3x3 convolution whose INPUT carries a folded per-channel shift t (a BatchNorm in front of a zero-padded
// convolution: the shift does not see the padding ring): entry idx = top | bottom<<1 | left<<2 | right<<3 sums the shift
// contribution of the taps that fall inside the image.  wf = [N][C][3][3] (already scaled by the output BN), cs = first
// input channel the shift applies to, ti = shift per channel.
void border_bias16(const std::vector<double>& wf, int N, int C, int cs, const std::vector<double>& ti, const std::vector<double>& bo,
                   std::vector<double>* b16 /* [16][N] */) {
    std::vector<double> tmap((size_t)N * 9, 0.0);
    const int nt = (int)ti.size();
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < nt; ++c) {
            const double* p = wf.data() + ((size_t)n * C + cs + c) * 9;
            for (int t = 0; t < 9; ++t) tmap[(size_t)n * 9 + t] += p[t] * ti[c];
        }
    b16->assign((size_t)16 * N, 0.0);
    for (int idx = 0; idx < 16; ++idx)
        for (int n = 0; n < N; ++n) {
            double acc = 0.0;
            for (int r = 0; r < 3; ++r) {
                if ((r == 0 && (idx & 1)) || (r == 2 && (idx & 2))) continue;
                for (int c = 0; c < 3; ++c) {
                    if ((c == 0 && (idx & 4)) || (c == 2 && (idx & 8))) continue;
                    acc += tmap[(size_t)n * 9 + r * 3 + c];
                }
            }
            (*b16)[(size_t)idx * N + n] = bo[n] + acc;
        }
}

// The 3x3 convolution of FPN level `level` of one head (FPN_DIM outputs, `cin` inputs, its output BatchNorm folded in) with the head's INPUT
// BatchNorm `in_bn` over the input channels [cs, cs + n) folded in exactly: scale into those weight columns, shift into the 16-case
// border bias table.  wf = [FPN_DIM][cin][3][3], b16 = [16][FPN_DIM].  Leafmap.forward, detector.py:194-197.
bool fold_head_input_bn(Weights& w, const std::string& head, int level, int in_bn, int cin, int cs, int n, std::vector<double>* wf,
                        std::vector<double>* b16) {
    const std::string up = head + ".upsamplers." + std::to_string(level);
    BnAffine in;
    std::vector<double> b;
    if (!bn_affine(w, head + ".in_bn." + std::to_string(in_bn), n, HEAD_BN_EPS, &in) ||
        !fold(w, up + ".0.weight", up + ".1", HEAD_BN_EPS, FPN_DIM, cin, 3, wf, &b)) return false;
    border_bias16(*wf, FPN_DIM, cin, cs, in.t, b, b16);
    for (int o = 0; o < FPN_DIM; ++o)
        for (int c = 0; c < n; ++c) {
            double* q = wf->data() + ((size_t)o * cin + cs + c) * 9;
            for (int t = 0; t < 9; ++t) q[t] *= in.s[c];
        }
    return true;
}

}  // namespace

int pack_weights(ftc_model* m, Weights& w) {
    const bool bf = m->precision != FTC_F32;      // a 16-bit speed mode (bf16 or fp16 operands): the fused / folded head variants exist
    const int cdt = m->split16 ? FTC_PRECISION_F16X3 : m->precision;      // storage of the MFMA weight operands (fp16x3: pre-split fp32 chunks)
    Blob& bl = m->blob;
    bool ok = true;
    std::vector<double> wf, b;
    auto conv_bn = [&](const std::string& name, const std::string& conv_key, const std::string& bn, double eps, int O, int I, int k) {
        if (!fold(w, conv_key, bn, eps, O, I, k, &wf, &b)) { ok = false; return; }
        const std::vector<double> km = kmajor(wf, O, I, k);
        bl.add_compute(name + ".w", km.data(), (int64_t)km.size(), cdt);
        bl.add_f32(name + ".b", b.data(), O);
    };
    const auto stages = backbone_blocks(m->size);
    const int c0 = stage_rows(m->size)[0].cin;
    // stem: [C0,3,3,3] -> [(r*3+s)*3+c][C0] fp32 (VALU kernel, always fp32)
    if (fold(w, "backbone.features.0.0.weight", "backbone.features.0.1", BACKBONE_BN_EPS, c0, 3, 3, &wf, &b)) {
        std::vector<double> sw((size_t)27 * c0);
        for (int o = 0; o < c0; ++o)
            for (int c = 0; c < 3; ++c)
                for (int t = 0; t < 9; ++t) sw[((size_t)t * 3 + c) * c0 + o] = wf[((size_t)o * 3 + c) * 9 + t];
        bl.add_f32("stem.w", sw.data(), (int64_t)sw.size());
        bl.add_f32("stem.b", b.data(), c0);
    } else ok = false;
    for (const auto& st : stages)
        for (const BlockSpec& blk : st) {
            const std::string p = blk.prefix + ".block";
            if (blk.fused) {
                if (blk.exp != blk.cin) {
                    conv_bn(p + ".0", p + ".0.0.weight", p + ".0.1", BACKBONE_BN_EPS, blk.exp, blk.cin, 3);
                    conv_bn(p + ".1", p + ".1.0.weight", p + ".1.1", BACKBONE_BN_EPS, blk.cout, blk.exp, 1);
                } else {
                    conv_bn(p + ".0", p + ".0.0.weight", p + ".0.1", BACKBONE_BN_EPS, blk.cout, blk.cin, 3);
                }
            } else {
                conv_bn(p + ".0", p + ".0.0.weight", p + ".0.1", BACKBONE_BN_EPS, blk.exp, blk.cin, 1);
                if (fold(w, p + ".1.0.weight", p + ".1.1", BACKBONE_BN_EPS, blk.exp, 1, 3, &wf, &b)) {          // depthwise [C,1,3,3] -> [9][C]
                    std::vector<double> dw((size_t)9 * blk.exp);
                    for (int c = 0; c < blk.exp; ++c)
                        for (int t = 0; t < 9; ++t) dw[(size_t)t * blk.exp + c] = wf[(size_t)c * 9 + t];
                    bl.add_f32(p + ".1.w", dw.data(), (int64_t)dw.size());
                    bl.add_f32(p + ".1.b", b.data(), blk.exp);
                } else ok = false;
                const TensorView *w1 = w.get(p + ".2.fc1.weight", {blk.squeeze, blk.exp, 1, 1}), *b1 = w.get(p + ".2.fc1.bias", {blk.squeeze}),
                                 *w2 = w.get(p + ".2.fc2.weight", {blk.exp, blk.squeeze, 1, 1}), *b2 = w.get(p + ".2.fc2.bias", {blk.exp});
                if (w1 && b1 && w2 && b2) {
                    bl.add_f32(p + ".2.w1", w1->data, (int64_t)blk.squeeze * blk.exp);                         // [S][C]
                    bl.add_f32(p + ".2.b1", b1->data, blk.squeeze);
                    std::vector<float> w2t((size_t)blk.squeeze * blk.exp);                                     // fc2 transposed [S][C]
                    for (int c = 0; c < blk.exp; ++c)
                        for (int s = 0; s < blk.squeeze; ++s) w2t[(size_t)s * blk.exp + c] = w2->data[(size_t)c * blk.squeeze + s];
                    bl.add_f32(p + ".2.w2t", w2t.data(), (int64_t)w2t.size());
                    bl.add_f32(p + ".2.b2", b2->data, blk.exp);
                } else ok = false;
                conv_bn(p + ".3", p + ".3.0.weight", p + ".3.1", BACKBONE_BN_EPS, blk.cout, blk.exp, 1);
            }
        }
    const int nfeat = (int)stages.size() + 1;
    const std::string hp = "backbone.features." + std::to_string(nfeat);
    const int clast = stages.back().back().cout;
    conv_bn(hp, hp + ".0.weight", hp + ".1", BACKBONE_BN_EPS, LAST_CHANNEL, clast, 1);
    const std::vector<int> taps = tap_dims(m->size);
    const int ntap = (int)taps.size();
    // FPN level 0 of all nine heads as ONE convolution over the shared 1/32 tap: each head's input BatchNorm is folded in
    // exactly -- scale into the weights, shift into a 16-entry border-case bias table.  Leafmap.forward i=0, detector.py:194-197.
    {
        const int C4 = taps[ntap - 1];
        std::vector<double> wm_all, b16_all((size_t)16 * NHEADS * FPN_DIM);
        wm_all.reserve((size_t)NHEADS * FPN_DIM * 9 * C4);
        for (int hi = 0; hi < NHEADS; ++hi) {
            std::vector<double> b16;
            if (!fold_head_input_bn(w, HEADS[hi].name, 0, ntap - 1, C4, 0, C4, &wf, &b16)) { ok = false; break; }
            const std::vector<double> km = kmajor(wf, FPN_DIM, C4, 3);
            wm_all.insert(wm_all.end(), km.begin(), km.end());
            for (int idx = 0; idx < 16; ++idx)
                for (int n = 0; n < FPN_DIM; ++n) b16_all[(size_t)idx * NHEADS * FPN_DIM + hi * FPN_DIM + n] = b16[(size_t)idx * FPN_DIM + n];
        }
        if (ok) {
            bl.add_compute("heads.L0.w", wm_all.data(), (int64_t)wm_all.size(), cdt);
            bl.add_f32("heads.L0.b", b16_all.data(), (int64_t)b16_all.size());                         // [16][9*192]
        }
    }
    // FPN levels 1.. and the input BatchNorms of the nine heads are stored head-major ([9][...]) so that one grouped launch
    // (ftc_op.groups = 9) covers all heads of a level.
    for (int i = 0; i < ntap - 1 && ok; ++i) {
        std::vector<float> sc((size_t)NHEADS * taps[i]), sh((size_t)NHEADS * taps[i]);
        for (int hi = 0; hi < NHEADS; ++hi) {
            BnAffine a;
            if (!bn_affine(w, std::string(HEADS[hi].name) + ".in_bn." + std::to_string(i), taps[i], HEAD_BN_EPS, &a)) { ok = false; break; }
            for (int c = 0; c < taps[i]; ++c) { sc[(size_t)hi * taps[i] + c] = (float)a.s[c]; sh[(size_t)hi * taps[i] + c] = (float)a.t[c]; }
        }
        bl.add_f32("heads.in_bn." + std::to_string(i) + ".scale", sc.data(), (int64_t)sc.size());
        bl.add_f32("heads.in_bn." + std::to_string(i) + ".shift", sh.data(), (int64_t)sh.size());
    }
    for (int i = 1; i < ntap && ok; ++i) {
        const int cin = FPN_DIM + taps[ntap - 1 - i];
        std::vector<double> wall, ball;
        for (int hi = 0; hi < NHEADS; ++hi) {
            const std::string name = HEADS[hi].name;
            if (!fold(w, name + ".upsamplers." + std::to_string(i) + ".0.weight", name + ".upsamplers." + std::to_string(i) + ".1", HEAD_BN_EPS,
                      FPN_DIM, cin, 3, &wf, &b)) { ok = false; break; }
            const std::vector<double> km = kmajor(wf, FPN_DIM, cin, 3);
            wall.insert(wall.end(), km.begin(), km.end());
            ball.insert(ball.end(), b.begin(), b.end());
        }
        if (!ok) break;
        bl.add_compute("heads.L" + std::to_string(i) + ".w", wall.data(), (int64_t)wall.size(), cdt);
        bl.add_f32("heads.L" + std::to_string(i) + ".b", ball.data(), (int64_t)ball.size());
    }
    if (ntap >= 2 && ok) {                  // (round 5: in the fp32 / fp16x3 plans too; the convolution then reads the fp32 tap itself)
        // Last level with the input BatchNorm of the backbone tap folded in exactly (as level 0 above): scale into the tap columns
        // of the weights, shift into a 16-case border bias table -- the convolution then reads the shared bf16 trunk copy of the
        // tap instead of nine batch-normed copies (FTC_FLAG_GROUP_IN2_SHARED + FTC_FLAG_BORDER_BIAS).
        const int i = ntap - 1, tc = taps[0], cin = FPN_DIM + tc;
        std::vector<double> wall, ball((size_t)NHEADS * 16 * FPN_DIM);
        for (int hi = 0; hi < NHEADS; ++hi) {
            std::vector<double> b16;
            if (!fold_head_input_bn(w, HEADS[hi].name, i, 0, cin, FPN_DIM, tc, &wf, &b16)) { ok = false; break; }
            const std::vector<double> km = kmajor(wf, FPN_DIM, cin, 3);
            wall.insert(wall.end(), km.begin(), km.end());
            std::copy(b16.begin(), b16.end(), ball.begin() + (size_t)hi * 16 * FPN_DIM);
        }
        if (ok) {
            bl.add_compute("heads.L" + std::to_string(i) + "f.w", wall.data(), (int64_t)wall.size(), cdt);
            bl.add_f32("heads.L" + std::to_string(i) + "f.b", ball.data(), (int64_t)ball.size());         // [9][16][192]
            if (bf && cin % 64 == 0) {
                // the same weights FRAGMENT-MAJOR for the weights-through-L1 kernel (FTC_FLAG_W_FRAG): per head
                // [6 row blocks][9 taps][cin/64][4 K groups][64 lanes][8]: lane L, element e = W[32 rb + (L & 31)][tap][64 cb + 16 g + 8 (L >> 5) + e]
                const int ncb = cin / 64;
                std::vector<double> wf2(wall.size());
                const size_t per_head = (size_t)FPN_DIM * 9 * cin;
                for (int hi = 0; hi < NHEADS; ++hi) {
                    const double* km = wall.data() + hi * per_head;
                    double* dst = wf2.data() + hi * per_head;
                    for (int rb = 0; rb < 6; ++rb)
                        for (int t = 0; t < 9; ++t)
                            for (int cb = 0; cb < ncb; ++cb)
                                for (int g = 0; g < 4; ++g)
                                    for (int L = 0; L < 64; ++L) {
                                        const size_t src = ((size_t)(rb * 32 + (L & 31)) * 9 + t) * cin + cb * 64 + g * 16 + (L >> 5) * 8;
                                        const size_t d = (((((size_t)rb * 9 + t) * ncb + cb) * 4 + g) * 64 + L) * 8;
                                        for (int e = 0; e < 8; ++e) dst[d + e] = km[src + e];
                                    }
                }
                bl.add_compute("heads.L" + std::to_string(i) + "f.wfrag", wf2.data(), (int64_t)wf2.size(), cdt);
            }
        }
    }
    // top convolutions (3x3, with bias, no BN): K-major [co][9][192]
    auto top = [&](const std::string& name, int co, std::vector<double>* km, std::vector<float>* bias) -> bool {
        const TensorView *tw = w.get(name + ".top_conv.0.weight", {co, FPN_DIM, 3, 3}), *tb = w.get(name + ".top_conv.0.bias", {co});
        if (!tw || !tb) return false;
        std::vector<double> wd((size_t)co * FPN_DIM * 9);
        for (size_t i = 0; i < wd.size(); ++i) wd[i] = (double)tw->data[i];
        *km = kmajor(wd, co, FPN_DIM, 3);
        bias->assign(tb->data, tb->data + co);
        return true;
    };
    std::vector<double> km;
    std::vector<float> tb;
    for (int hi : {0, 1, 8}) {
        if (!ok || !top(HEADS[hi].name, HEADS[hi].out_dim, &km, &tb)) { ok = false; break; }
        bl.add_compute(std::string(HEADS[hi].name) + ".top_conv.w", km.data(), (int64_t)km.size(), cdt);
        bl.add_f32(std::string(HEADS[hi].name) + ".top_conv.b", tb.data(), (int64_t)tb.size());
    }
    if (ok) {   // the six one-channel heads whose heat-map channels are consecutive (textline, separator, code1/2/4/8 -> channels 4..9)
        std::vector<double> w6;
        std::vector<float> b6;
        for (int hi = 2; hi < 8; ++hi) {
            if (!top(HEADS[hi].name, 1, &km, &tb)) { ok = false; break; }
            w6.insert(w6.end(), km.begin(), km.end());
            b6.push_back(tb[0]);
        }
        if (ok) {
            bl.add_compute("heads.top6.w", w6.data(), (int64_t)w6.size(), cdt);
            bl.add_f32("heads.top6.b", b6.data(), (int64_t)b6.size());
        }
    }
    if (ok) {
        // The eight map heads' top convolutions as per-pixel tap matrices for the fused last-level epilogue (FTC_FLAG_TOP_FUSE +
        // FTC_OP_TAPSUM): row tap*Co + o of head g = top_conv weight [o, :, r, s], 32 rows zero padded.
        std::vector<double> wt((size_t)(NHEADS - 1) * 32 * FPN_DIM, 0.0);
        std::vector<float> bias;
        std::vector<int32_t> omap;
        for (int g = 0; g < NHEADS - 1; ++g) {
            const int co = HEADS[g].out_dim, ch0 = HEADS[g].ch0;
            if (!top(HEADS[g].name, co, &km, &tb)) { ok = false; break; }
            for (int o = 0; o < co; ++o) {
                for (int t = 0; t < 9; ++t)
                    for (int c = 0; c < FPN_DIM; ++c) wt[((size_t)g * 32 + t * co + o) * FPN_DIM + c] = km[((size_t)o * 9 + t) * FPN_DIM + c];
                bias.push_back(tb[o]);
                omap.insert(omap.end(), {g, o, co, (ch0 == 0 ? 0 : ch0 + 1) + o});
            }
        }
        if (ok) {
            if (!bf) {                           // fp32 / fp16x3 plans: the epilogue multiplies in fp32 FMA (conv_epilogue_topfuse_f32): a plain fp32 matrix
                std::vector<float> wf(wt.begin(), wt.end());
                bl.add_f32("heads.top8.wt", wf.data(), (int64_t)wf.size());
            } else {
                bl.add_compute("heads.top8.wt", wt.data(), (int64_t)wt.size(), cdt);
            }
            bl.add_f32("heads.top8.b", bias.data(), (int64_t)bias.size());
            std::memcpy(bl.add("heads.top8.map", (int64_t)omap.size() * 4), omap.data(), omap.size() * 4);
        }
    }
    if (!ok) return ftc_set_error(FTC_ERR_INVALID, "ftc_create: " + (w.missing.empty() ? std::string("weight packing failed") : w.missing));
    const auto refuse_range = [&] {
        return ftc_set_error(FTC_ERR_INVALID, "ftc_create: folded weight tensor '" + bl.out_of_range + "' holds a value that is not finite or lies beyond +-65504: "
                                              "FTC_PRECISION_F16X3 would clamp it where the reference does not (use FTC_F32 for this checkpoint)");
    };
    if (!bl.out_of_range.empty()) return refuse_range();
    // SimpleDecoder (models/detector.py:232-254), optional: three MLPs Linear(100,2048,no bias) -> BatchNorm1d -> GELU -> Linear(2048,2048,
    // no bias) -> BatchNorm1d -> GELU -> Linear(2048, modulo).  Eval-mode BatchNorm1d (eps 1e-5) folds into the Linear before it; a Linear
    // weight [out][in] already is the K-major layout of a 1x1 convolution.  The first layer's K is zero-padded 100 -> 128.
    if (w.t.count("decoder.blocks.0.0.weight")) {
        for (int i = 0; i < 3 && ok; ++i) {
            const std::string p = "decoder.blocks." + std::to_string(i), q = "decoder." + std::to_string(i);
            const int mod = DECODER_MODULO[i];
            const TensorView *w0 = w.get(p + ".0.weight", {DECODER_MID, FEATURE_DIM}), *w1 = w.get(p + ".3.weight", {DECODER_MID, DECODER_MID}),
                             *w2 = w.get(p + ".6.weight", {mod, DECODER_MID}), *b2 = w.get(p + ".6.bias", {mod});
            BnAffine a0, a1;
            if (!w0 || !w1 || !w2 || !b2 || !bn_affine(w, p + ".1", DECODER_MID, HEAD_BN_EPS, &a0) || !bn_affine(w, p + ".4", DECODER_MID, HEAD_BN_EPS, &a1)) { ok = false; break; }
            std::vector<double> l0((size_t)DECODER_MID * DECODER_KPAD, 0.0), l1((size_t)DECODER_MID * DECODER_MID), l2((size_t)mod * DECODER_MID);
            for (int o = 0; o < DECODER_MID; ++o) {
                for (int c = 0; c < FEATURE_DIM; ++c) l0[(size_t)o * DECODER_KPAD + c] = (double)w0->data[(size_t)o * FEATURE_DIM + c] * a0.s[o];
                for (int c = 0; c < DECODER_MID; ++c) l1[(size_t)o * DECODER_MID + c] = (double)w1->data[(size_t)o * DECODER_MID + c] * a1.s[o];
            }
            for (size_t j = 0; j < l2.size(); ++j) l2[j] = (double)w2->data[j];
            bl.add_compute(q + ".l0.w", l0.data(), (int64_t)l0.size(), cdt);
            bl.add_f32(q + ".l0.b", a0.t.data(), DECODER_MID);
            bl.add_compute(q + ".l1.w", l1.data(), (int64_t)l1.size(), cdt);
            bl.add_f32(q + ".l1.b", a1.t.data(), DECODER_MID);
            bl.add_compute(q + ".l2.w", l2.data(), (int64_t)l2.size(), cdt);
            bl.add_f32(q + ".l2.b", b2->data, mod);
        }
        if (!ok) return ftc_set_error(FTC_ERR_INVALID, "ftc_create: decoder: " + (w.missing.empty() ? std::string("weight packing failed") : w.missing));
        if (!bl.out_of_range.empty()) return refuse_range();
        m->has_decoder = true;
    }
    return FTC_OK;
}

}  // namespace ftc_model_detail
