// The plan builder behind ftc_forward (once per input shape and switch setting): the plan switches, the decision of every backbone block's
// form, the op list with its liveness-based activation arena, and the measured kernel selection: what a table key is and which hint an op
// adopts are decided here alone (ftc_conv_signature / ftc_tune_ops give the same answers to the train step and the tuner).
// Host-only code: no kernels here.  Compiled with -ffp-contract=off like pack.hip: the flops / bytes figures of ftc_op_info are sums of
// products in float64 and stay the same between builds.
#include <cstdlib>
#include <cstring>

#include "model_net.h"

namespace ftc_model_detail {

namespace {

// ---- measured kernel selection ----------------------------------------------------------------------
struct TuneEntry { const char* sig; int aux0; };
const TuneEntry kTuning[] = {
#include "build/tuning_table.inc"       // written by build.py from tuning_gfx950.json
    {nullptr, 0}};

// The measured choices by signature, with the entries of the FTC_TUNING_OVERRIDE file, if any, merged in: built when the first plan that
// is tuned asks for it (a process that keeps FTC_NO_TUNING set never opens the file)
const std::map<std::string, int>& tuning_table() {
    static const std::map<std::string, int> table = [] {
        std::map<std::string, int> t;
        for (const TuneEntry* e = kTuning; e->sig; ++e) t[e->sig] = e->aux0;
        const char* path = nullptr;
        read_plan_options(&path);
        if (FILE* f = path ? std::fopen(path, "r") : nullptr) {
            char sig[192];
            int v;
            int n = 0;
            while (std::fscanf(f, "%191s %d", sig, &v) == 2) { t[sig] = v; ++n; }
            std::fclose(f);
            std::fprintf(stderr, "[ftc] FTC_TUNING_OVERRIDE: %d entries from %s\n", n, path);
        }
        return t;
    }();
    return table;
}

std::string conv_signature(const ftc_op& o, bool strip_split = false) {
    char buf[192];
    // fp16 operands run the same kernels at the same rate as bf16: they share the measured table (dtype 2 looks up as 1)
    auto d = [](int dt) { return dt == FTC_F16 ? (int)FTC_BF16 : dt; };
    int n = std::snprintf(buf, sizeof buf, "w%di%do%d_B%d_%dx%d_c%dof%d_n%dof%d_k%ds%d_f%d_a%d", d(o.w_dtype), d(o.in_dtype), d(o.out_dtype), o.B, o.H, o.W,
                          o.Cin, o.Cin_total, o.Cout, o.Cout_total, o.ksize, o.stride, (strip_split ? (o.flags & ~FTC_FLAG_SPLIT16) : o.flags) & ~(FTC_FLAG_KBLOCK32 | FTC_FLAG_PRESPLIT), o.act);      // (KBLOCK32: where the 16-bit copy goes, not which kernel is fastest)
    if (o.groups > 1) std::snprintf(buf + n, sizeof buf - n, "_g%d", o.groups);
    return buf;
}

// Returns how many ops took a table entry
int apply_tuning(ftc_op* ops, int n_ops, const PlanOptions& opt) {
    if (opt.no_tuning) return 0;
    const std::map<std::string, int>& table = tuning_table();
    int n = 0;
    for (int i = 0; i < n_ops; ++i) {
        ftc_op& o = ops[i];
        if (o.kind != FTC_OP_CONV) continue;
        auto it = table.find(conv_signature(o));
        if (it == table.end() && (o.flags & FTC_FLAG_SPLIT16)) it = table.find(conv_signature(o, true));     // fp16x3 without its own measurement: the fp32 choice
        if (it == table.end() || !it->second) continue;
        // A table entry is a HINT measured for one flag combination; the signature drops flags that do not change which kernel is fastest
        // (KBLOCK32, PRESPLIT) and fp16x3 falls back to the fp32 entry, so an entry can name a kernel that is not legal for THIS op
        // (e.g. a 144-pixel fp16x3 tile without pre-split operands under FTC_NO_PRESPLIT / FTC_NO_MBSLICE_X3).  Adopt it only if the op
        // validates with it; otherwise the default selection stands.
        const int keep = o.aux0;
        o.aux0 = it->second;
        if (conv_validate(o) != nullptr) o.aux0 = keep;
        else ++n;
    }
    return n;
}

}  // namespace

// ---- plan switches: the one place that reads the environment ---------------------------------------------------------------------
PlanOptions read_plan_options(const char** tuning_override) {
    auto on = [](const char* k) { const char* v = std::getenv(k); return v && *v && std::strcmp(v, "0") != 0; };
    PlanOptions o;
    o.no_mbslice = on("FTC_NO_MBSLICE");
    o.no_mbslice_x3 = on("FTC_NO_MBSLICE_X3");
    o.no_mbband = on("FTC_NO_MBBAND");
    if (const char* e = std::getenv("FTC_MBSLICE_96")) o.mbslice_96 = e[0] != '0';
    if (const char* e = std::getenv("FTC_MBSLICE_MINWG")) o.mbslice_minwg = std::atoi(e);
    o.no_fmbfuse = on("FTC_NO_FMBFUSE");
    o.no_fmbfuse_x3 = on("FTC_NO_FMBFUSE_X3");
    o.fmbfuse_all = on("FTC_FMBFUSE_ALL");
    o.no_kblock = on("FTC_NO_KBLOCK");
    o.no_x3fold = on("FTC_NO_X3FOLD");
    o.no_presplit = on("FTC_NO_PRESPLIT");
    o.no_topfuse = on("FTC_NO_TOPFUSE");
    o.no_topfuse32 = on("FTC_NO_TOPFUSE32");
    o.no_upfuse = on("FTC_NO_UPFUSE");
    o.no_upfuse32 = on("FTC_NO_UPFUSE32");
    o.no_upfuse32_l2 = on("FTC_NO_UPFUSE32_L2");
    o.no_bnfold = on("FTC_NO_BNFOLD");
    o.no_bnfold32 = on("FTC_NO_BNFOLD32");
    o.no_wl1 = on("FTC_NO_WL1");
    o.no_tuning = on("FTC_NO_TUNING");
    if (const char* e = std::getenv("FTC_PLAN_SHRINK_BUF")) o.shrink_buf = *e ? std::atoi(e) : -1;
    // FTC_TUNING_OVERRIDE=<file of "signature aux0" lines>: entries replacing / extending the compiled-in table (tuning experiments without
    // a rebuild, e.g. tools/lanes_tuning.py: choices measured for the two-lane steady state instead of the kernel alone).  Not a member: read
    // once per process, for tuning_table.
    static const std::string override_path = [] { const char* p = std::getenv("FTC_TUNING_OVERRIDE"); return std::string(p ? p : ""); }();
    if (tuning_override) *tuning_override = override_path.empty() ? nullptr : override_path.c_str();
    return o;
}

namespace {

// ---- plan builder ---------------------------------------------------------------------------------------
struct Buf { int64_t nbytes; int first = 1 << 30, last = -1; int64_t offset = -1; };
struct R {                    // symbolic operand: arena buffer (+ byte offset inside it) | weights | input | outputs
    int kind = 0;             // 0 none, 1 buf, 2 weights, 3 input, 4 heatmap, 5 features
    int64_t v = 0, extra = 0;
    explicit operator bool() const { return kind != 0; }
};
const R IMAGE{3, 0, 0}, HEATMAP{4, 0, 0}, FEATURES{5, 0, 0};
struct SymOp {
    ftc_op o{};
    R in, in2, out, w, w2, bias, bias2, scale, shift, aux, out2;
};

struct ConvOpt {
    int cout_total = 0, cout_off = 0;
    R residual, se, out2, wsets;
    int res_dt = 0, extra_flags = 0, groups = 1;
    int64_t w_off = 0, b_off = 0;
};

// The numeric mode of a model, as the plan sees it
struct Mode {
    static constexpr int trunk = FTC_F32;      // residual trunk + taps stay fp32
    int act;         // dtype of the activations between GEMMs and of the MFMA weight operands: the model's precision (fp16x3: fp32)
    bool dual;       // 16-bit speed mode (bf16 or fp16 operands): every trunk tensor is written together with a 16-bit copy by the
                     // producing epilogue; the next GEMM reads the copy
    bool x3;         // fp16x3 plan: fp32 tensors, every product as three fp16 MFMAs (FTC_FLAG_SPLIT16 on every GEMM-shaped op)
    int gemm_in;     // dtype the GEMMs read the trunk in
    int split;       // FTC_FLAG_SPLIT16 in the fp16x3 plan, else 0
    explicit Mode(const ftc_model* m)
        : act(m->precision), dual(m->precision != FTC_F32), x3(m->split16 && m->precision == FTC_F32), gemm_in(dual ? act : trunk),
          split(x3 ? FTC_FLAG_SPLIT16 : 0) {}
};

// Everything the emission of one backbone block needs, decided once (Builder::decide_block)
enum class BlockForm {
    FUSED_PLAIN,     // Fused-MBConv without expansion: one 3x3 convolution
    FMB_ONE,         // Fused-MBConv with expansion in ONE launch (FTC_OP_FMBCONV, csrc/fused_mbconv.hip)
    FMB_TWO,         // ... as 3x3 expand + 1x1 project
    MB_SLICED,       // MBConv: expand + depthwise + SE partial sums in one launch (FTC_OP_MBHEAD, csrc/mbconv_slice.hip), SE, project
    MB_EXPAND_DW,    // MBConv: expand, depthwise, SE, project
};
struct BlockPlan {
    BlockForm form = BlockForm::FUSED_PLAIN;
    int h = 0, w = 0, ho = 0, wo = 0;   // the block's input and output map
    int band_rows = -1, nbands = 1;     // MB_SLICED: output rows per band (0 = the whole map), bands per image
    int mb_slice = 0;                   // MB_SLICED: expanded channels per workgroup
    int P = 0;                          // MBConv: partial SE sums per image and channel
    bool next_sliced = false;           // the next block is MB_SLICED: it reads this block's 16-bit / pre-split trunk copy
    bool out_blocked = false;           // ... and streams that copy in 32-channel planes (FTC_FLAG_KBLOCK32)
    bool foldse = false;                // MBConv: the SE op writes the project weights scaled per image
    bool presplit = false;              // fp16x3, MB_SLICED: the head writes d pre-split and the project convolution reads it so
};

class Builder {
public:
    Builder(ftc_model* m, int B, int H, int W, bool nchw, const PlanOptions& opt) : m_(m), B(B), H(H), W(W), nchw_(nchw), opt_(opt), md_(m) {}
    int build(ModelPlan* out);
    int build_decoder(ModelPlan* out);          // constructed with B = 1, H = rows, W = 1

private:
    struct Tap { R buf; int c, h, w, dt; };
    struct Level;
    static constexpr int TW = 20;               // floats per pixel of the fused top convolutions' tap tensor (9 * 2 outputs, padded)
    static constexpr int NMAP = NHEADS - 1;     // the map heads (all but `feature`)

    ftc_model* m_;
    int B, H, W;
    bool nchw_;
    const PlanOptions opt_;
    const Mode md_;
    std::vector<SymOp> ops_;
    std::vector<OpMeta> meta_;
    std::vector<Buf> bufs_;
    std::string err_;
    // the trunk while the backbone is emitted: fp32 tensor, its 16-bit / pre-split copy (or none), map size, copy in 32-channel planes
    R x_, xb_;
    int h_ = 0, w_ = 0;
    bool in_blocked_ = false;
    std::vector<Tap> taps_;
    std::vector<R> tap_copies_;                 // 16-bit trunk copies of the backbone taps (16-bit modes), same order

    static int esize(int dt) { return dt == FTC_F32 ? 4 : 2; }
    R buf(int64_t nelem, int dt) { bufs_.push_back({align_up(nelem * esize(dt))}); return {1, (int64_t)bufs_.size() - 1, 0}; }
    R sub(const R& b, int64_t off) const { return {1, b.v, b.extra + off}; }
    // the op as op_extents reads it: the int fields, and which operands are given
    static ftc_op form_of(const SymOp& s) {
        ftc_op o = s.o;
        for (int i = 0; i < FTC_NUM_OPERANDS; ++i) (&o.in)[i].base = (&s.in)[i] ? FTC_BASE_WORKSPACE : FTC_BASE_NULL;
        return o;
    }
    // A pure scratch operand of the op being built (its int fields and the operands its form depends on are set): as many bytes as the op touches through it
    R scratch(const SymOp& s, int operand) {
        OpExtents e;
        if (const char* refused = op_extents(form_of(s), &e)) { if (err_.empty()) err_ = refused; return {}; }
        bufs_.push_back({align_up(e.bytes[operand])});
        return {1, (int64_t)bufs_.size() - 1, 0};
    }
    R wref(const std::string& name, int64_t off = 0) {
        auto it = m_->blob.table.find(name);
        if (it == m_->blob.table.end()) { if (err_.empty()) err_ = "packed weight '" + name + "' missing"; return {}; }
        return {2, it->second + off, 0};
    }
    bool has_w(const std::string& name) const { return m_->blob.table.count(name) != 0; }
    R gin() const { return md_.dual ? xb_ : x_; }          // GEMM-side view of the trunk
    // In 16-bit modes every trunk tensor gets a 16-bit copy; in the fp16x3 plan a block whose output feeds a fused MBConv head gets a second,
    // PRE-SPLIT copy of its fp32 trunk tensor (hi | lo halves per 16-byte chunk: what csrc/mbconv_slice_x3.hip streams by DMA) -- `want_copy`
    void trunk(int64_t nelem, R* t, R* tb, bool want_copy = false) {
        *t = buf(nelem, Mode::trunk);
        *tb = md_.dual ? buf(nelem, md_.act) : (md_.x3 && want_copy) ? buf(nelem, FTC_F32) : R();
    }
    // an op of `kind` on B images with its geometry set; everything else zero
    SymOp geom(int kind, int h, int w, int ho, int wo, int cin = 0, int cout = 0, int k = 0, int stride = 0) const {
        SymOp s;
        ftc_op& o = s.o;
        o.kind = kind; o.B = B; o.H = h; o.W = w; o.Ho = ho; o.Wo = wo; o.Cin = cin; o.Cout = cout; o.ksize = k; o.stride = stride;
        return s;
    }
    void emit(const OpMeta& meta, const SymOp& s) {
        const int idx = (int)ops_.size();
        for (const R* r : {&s.in, &s.in2, &s.out, &s.aux, &s.scale, &s.out2, &s.w, &s.w2})
            if (r->kind == 1) { Buf& b = bufs_[r->v]; b.first = std::min(b.first, idx); b.last = std::max(b.last, idx); }
        ops_.push_back(s);
        meta_.push_back(meta);
    }
    void conv(const std::string& name, R x, int xdt, int h, int w, int cin, int cin_total, int cin_off, const std::string& wname, int cout, int k,
              int stride, int act, R out, int odt, const ConvOpt& c = ConvOpt()) {
        const int Ho = (h - 1) / stride + 1, Wo = (w - 1) / stride + 1, wdt = md_.act;
        int flags = (c.residual ? FTC_FLAG_RESIDUAL : 0) | (c.se ? FTC_FLAG_SE_SCALE : 0) | c.extra_flags | md_.split;
        const double macs = (double)c.groups * B * Ho * Wo * cout * cin * k * k;
        double byt = (double)c.groups * ((double)B * h * w * cin * esize(xdt) + (double)B * Ho * Wo * cout * esize(odt) + (double)cout * cin * k * k * esize(wdt));
        if (c.residual) byt += (double)B * Ho * Wo * cout * esize(c.res_dt);
        if (c.out2) byt += (double)B * Ho * Wo * cout * 2;
        if (c.wsets) { flags |= FTC_FLAG_W_PER_IMAGE; byt += (double)(B - 1) * cout * cin * k * k * esize(wdt); }
        SymOp s = geom(FTC_OP_CONV, h, w, Ho, Wo, cin, cout, k, stride);
        ftc_op& o = s.o;
        o.flags = flags; o.act = act; o.in_dtype = xdt; o.out_dtype = odt; o.w_dtype = wdt;
        o.Cin_total = cin_total; o.cin_off = cin_off; o.Cout_total = c.cout_total ? c.cout_total : cout; o.cout_off = c.cout_off;
        o.res_dtype = c.res_dt; o.groups = c.groups > 1 ? c.groups : 0;
        s.in = x; s.in2 = c.residual; s.out = out; s.w = c.wsets ? c.wsets : wref(wname + ".w", c.w_off); s.bias = wref(wname + ".b", c.b_off);
        s.scale = c.se; s.out2 = c.out2;
        emit({name, "conv" + std::to_string(k) + "x" + std::to_string(k), 2.0 * macs, byt}, s);
    }

    int mb_slice_of(const BlockSpec& blk, int bh, int bw) const;
    int sliced_band_rows(const BlockSpec& blk, int bh, int bw, int mb_slice) const;
    bool fmb_one_launch(const BlockSpec& blk, int bh, int bw) const;
    BlockPlan decide_block(const BlockSpec& blk, int h, int w, bool has_copy, const BlockPlan* next) const;

    void emit_stem(int c0);
    void emit_block(const BlockSpec& blk, const BlockPlan& d);
    void emit_fmb_one(const BlockSpec& blk, const BlockPlan& d, R y, R yb);
    void emit_mb_head(const BlockSpec& blk, const BlockPlan& d, R dw, R part);
    void emit_mb_expand_dw(const BlockSpec& blk, const BlockPlan& d, R dw, R part);
    void emit_se_project(const BlockSpec& blk, const BlockPlan& d, R dw, R part, R y, const ConvOpt& tail);
    void emit_last_1x1(int clast, int nfeat);
    void emit_heads();
    void level_input(Level& lv);
    void level_conv(const Level& lv, const std::string& name, int g0, int ng, R outr, bool top);
    void emit_top_convs(R y, int yh, int yw);
    void emit_nms(int mh, int mw);
    int finish(ModelPlan* out, int mh, int mw);
};

// ---- the decision of a block's form ------------------------------------------------------------------------------
// Slice width of a block's fused head: 64 (fp32 tensors), 128, or -- whole-map blocks whose 128-channel slices leave more than a fifth of the 256
// CUs without a workgroup while 96-channel slices still fit one round (stage 6 at batch 8: 192 -> 256 workgroups) -- 96.  FTC_MBSLICE_96=0: never.
int Builder::mb_slice_of(const BlockSpec& blk, int bh, int bw) const {
    if (md_.x3) return FTC_MBHEAD_SLICE_F32;
    if (ftc_mbhead_band_rows(bh, bw) != 0 || blk.exp % 96 != 0 || !opt_.mbslice_96) return FTC_MBHEAD_SLICE;
    const int w128 = B * (blk.exp / 128), w96 = B * (blk.exp / 96);
    return (w128 <= 204 && w96 <= 256) ? 96 : FTC_MBHEAD_SLICE;
}

// Low-resolution MBConv stages (24x24 maps at 768x768: stages 6-7), 16-bit and fp16x3 plans: expand + depthwise + squeeze + the block's share
// of the SE fc1 layer in ONE launch, a workgroup per (image, mb_slice expanded channels) -- csrc/mbconv_slice.hip; the expanded tensor never
// leaves the CU.  FTC_NO_MBSLICE=1: the three-kernel form; FTC_MBSLICE_MINWG: workgroups below which the three-kernel form is kept
// (small batches leave most CUs without a slice).  bh, bw = the block's INPUT map.  Maps of more than 576 pixels -- the 48x48 stages 4-5 --
// run in bands of R output rows: returns R, 0 = the whole map, -1 = not sliced.
int Builder::sliced_band_rows(const BlockSpec& blk, int bh, int bw, int mb_slice) const {
    if (blk.fused || !(md_.dual || md_.x3) || blk.stride != 1 || blk.squeeze > FTC_MBHEAD_MAX_SQUEEZE || opt_.no_mbslice) return -1;
    if (md_.x3 && opt_.no_mbslice_x3) return -1;
    const int R = ftc_mbhead_band_rows(bh, bw);
    if (R < 0 || (R > 0 && opt_.no_mbband)) return -1;
    ftc_op t{};
    t.in_dtype = t.out_dtype = t.w_dtype = md_.act; t.stride = blk.stride; t.ksize = 3; t.H = t.Ho = bh; t.W = t.Wo = bw;
    t.Cin = blk.cin; t.Cout = blk.exp; t.aux1 = R; t.flags = md_.split;
    t.Cout_total = mb_slice;
    // (fp16x3, stage 5 at batch 8 -- 960 workgroups, every 64-channel slice re-streams its image's x: 143 us against 80 + 57 for the two kernels it
    //  replaces; kept all the same: its pre-split output saves the project convolution 10 us and the pair moves 113 MB less through HBM)
    return ftc_mbhead_legal(t) && B * ftc_mbhead_bands(t) * (blk.exp / mb_slice) >= opt_.mbslice_minwg ? R : -1;
}

// Fused-MBConv blocks with expansion, 16-bit and fp16x3 plans, stride 1: one launch (FTC_OP_FMBCONV) where the shape is one the kernel holds.
// The expanded tensor (151 MB per stage-2 block at batch 8) is neither written nor read back.  FTC_NO_FMBFUSE=1: the two-launch form.
bool Builder::fmb_one_launch(const BlockSpec& blk, int bh, int bw) const {
    if (!blk.fused || blk.exp == blk.cin || !(md_.dual || md_.x3) || blk.stride != 1 || opt_.no_fmbfuse) return false;
    if (md_.x3 && opt_.no_fmbfuse_x3) return false;
    // Measured (tools/fmbconv_bench.py, batch 8): the one-launch form wins where the 3x3 runs K steps of 64 (Cin % 64 == 0: stage 2, 174-182 us
    // against 126 + 65) and loses on stage 3 (Cin = 96: K steps of 32, twice the barriers per FLOP: 116-135 us against 75 + 28.5).
    // FTC_FMBFUSE_ALL=1: every shape the kernel holds.
    if (blk.cin % 64 != 0 && !opt_.fmbfuse_all) return false;
    ftc_op t{};
    t.in_dtype = t.w_dtype = md_.x3 ? FTC_F32 : md_.act; t.out_dtype = Mode::trunk; t.res_dtype = Mode::trunk; t.ksize = 3; t.stride = 1;
    t.H = t.Ho = bh; t.W = t.Wo = bw; t.B = B;
    t.Cin = t.Cin_total = blk.cin; t.Cout = t.Cout_total = blk.cout; t.aux1 = blk.exp; t.act = FTC_ACT_SILU;
    t.flags = (blk.residual ? FTC_FLAG_RESIDUAL : 0) | md_.split;
    return ftc_fmbconv_legal(t);
}

// h, w = the block's input map; has_copy: the block's input has a 16-bit / pre-split copy for a fused head to stream (fp16x3: the stem
// writes none); next = the decision of the block after it, or null.
BlockPlan Builder::decide_block(const BlockSpec& blk, int h, int w, bool has_copy, const BlockPlan* next) const {
    BlockPlan d;
    d.h = h; d.w = w; d.ho = (h - 1) / blk.stride + 1; d.wo = (w - 1) / blk.stride + 1;
    d.next_sliced = next && next->form == BlockForm::MB_SLICED;
    // the consumer of this block's 16-bit copy is the next block's expand GEMM: FTC_OP_MBHEAD streams it in 32-channel planes
    d.out_blocked = md_.dual && d.next_sliced && blk.cout % 32 == 0 && !opt_.no_kblock;
    if (blk.fused) {
        // (FTC_OP_FMBCONV writes its trunk copy as plain NHWC only: not in front of a fused head.  No s / m / l / xl table has that sequence.)
        d.form = blk.exp == blk.cin ? BlockForm::FUSED_PLAIN
                 : fmb_one_launch(blk, h, w) && !d.next_sliced && !d.out_blocked ? BlockForm::FMB_ONE : BlockForm::FMB_TWO;
        return d;
    }
    d.mb_slice = mb_slice_of(blk, h, w);
    d.band_rows = has_copy ? sliced_band_rows(blk, h, w, d.mb_slice) : -1;
    const bool slice = d.band_rows >= 0;
    d.form = slice ? BlockForm::MB_SLICED : BlockForm::MB_EXPAND_DW;
    d.nbands = d.band_rows > 0 ? (h + d.band_rows - 1) / d.band_rows : 1;
    const int th = blk.stride == 1 ? 8 : 4;
    d.P = slice ? d.nbands * (blk.exp / d.mb_slice) : ((d.ho + th - 1) / th) * ((d.wo + 7) / 8);
    // 16-bit modes: the SE op also writes the project weights scaled per image, so that the project convolution streams both
    // operands by DMA instead of rescaling activations while staging them.  Needs a 64-pixel tile that divides the image.
    // (fp16x3 plan: the same with pre-split fp32 chunks -- FTC_NO_X3FOLD=1 keeps the gate in the project convolution's staging)
    d.foldse = (md_.dual || (md_.x3 && !opt_.no_x3fold)) && (d.ho * d.wo) % 64 == 0 && blk.exp % 8 == 0;
    // fp16x3: the head writes d PRE-SPLIT when its only reader, the project convolution, runs on folded weights (no SE scale on the activations)
    d.presplit = md_.x3 && slice && d.foldse && !opt_.no_presplit;
    return d;
}

// ---- emitters -----------------------------------------------------------------------------------------------------
void Builder::emit_stem(int c0) {
    h_ = (H - 1) / 2 + 1; w_ = (W - 1) / 2 + 1;
    trunk((int64_t)B * h_ * w_ * c0, &x_, &xb_);
    SymOp s = geom(FTC_OP_STEM, H, W, h_, w_, 3, c0, 3, 2);
    ftc_op& o = s.o;
    o.flags = nchw_ ? FTC_FLAG_IN_NCHW : 0; o.act = FTC_ACT_SILU; o.in_dtype = FTC_F32; o.out_dtype = Mode::trunk;
    o.w_dtype = md_.dual ? md_.act : 0;                  // STEM: dtype of the 16-bit trunk copy (out2)
    s.in = IMAGE; s.out = x_; s.out2 = xb_; s.w = wref("stem.w"); s.bias = wref("stem.b");
    emit({"backbone.features.0", "stem", 2.0 * B * h_ * w_ * c0 * 27,
          (double)B * H * W * 3 * 4 + (double)B * h_ * w_ * c0 * (esize(Mode::trunk) + (md_.dual ? 2 : 0))}, s);
}

void Builder::emit_block(const BlockSpec& blk, const BlockPlan& d) {
    const std::string p = blk.prefix + ".block";
    const int T = Mode::trunk, A = md_.act, G = md_.gemm_in;
    R y, yb;
    trunk((int64_t)B * d.ho * d.wo * blk.cout, &y, &yb, d.next_sliced);
    ConvOpt tail;
    tail.residual = blk.residual ? x_ : R(); tail.res_dt = T; tail.out2 = yb;
    if (d.out_blocked) tail.extra_flags |= FTC_FLAG_KBLOCK32;
    switch (d.form) {
    case BlockForm::FUSED_PLAIN:
        conv(p + ".0", gin(), G, d.h, d.w, blk.cin, blk.cin, 0, p + ".0", blk.cout, 3, blk.stride, FTC_ACT_SILU, y, T, tail);
        break;
    case BlockForm::FMB_ONE:
        emit_fmb_one(blk, d, y, yb);
        break;
    case BlockForm::FMB_TWO: {
        const R e = buf((int64_t)B * d.ho * d.wo * blk.exp, A);
        conv(p + ".0", gin(), G, d.h, d.w, blk.cin, blk.cin, 0, p + ".0", blk.exp, 3, blk.stride, FTC_ACT_SILU, e, A);
        conv(p + ".1", e, A, d.ho, d.wo, blk.exp, blk.exp, 0, p + ".1", blk.cout, 1, 1, FTC_ACT_NONE, y, T, tail);
        break;
    }
    case BlockForm::MB_SLICED:
    case BlockForm::MB_EXPAND_DW: {
        const bool slice = d.form == BlockForm::MB_SLICED;
        const R dw = buf((int64_t)B * d.ho * d.wo * blk.exp, A);
        const R part = buf((int64_t)B * d.P * (slice ? blk.squeeze : blk.exp), FTC_F32);
        if (slice) emit_mb_head(blk, d, dw, part);
        else emit_mb_expand_dw(blk, d, dw, part);
        emit_se_project(blk, d, dw, part, y, tail);
        break;
    }
    }
    x_ = y; xb_ = yb; h_ = d.ho; w_ = d.wo;
    in_blocked_ = d.out_blocked;
}

void Builder::emit_fmb_one(const BlockSpec& blk, const BlockPlan& d, R y, R yb) {
    const std::string p = blk.prefix + ".block";
    const int T = Mode::trunk, G = md_.gemm_in;
    const R res = blk.residual ? x_ : R();
    SymOp s = geom(FTC_OP_FMBCONV, d.h, d.w, d.ho, d.wo, blk.cin, blk.cout, 3, 1);
    ftc_op& o = s.o;
    o.act = FTC_ACT_SILU; o.in_dtype = G; o.out_dtype = T; o.w_dtype = md_.act; o.res_dtype = T;
    o.flags = (res ? FTC_FLAG_RESIDUAL : 0) | md_.split;
    o.Cin_total = blk.cin; o.Cout_total = blk.cout; o.aux1 = blk.exp;
    s.in = gin(); s.in2 = res; s.out = y; s.out2 = yb; s.w2 = wref(p + ".0.w"); s.bias2 = wref(p + ".0.b"); s.w = wref(p + ".1.w"); s.bias = wref(p + ".1.b");
    const double px = (double)B * d.h * d.w;
    emit({p + ".0+1", "conv3x3+conv1x1", 2.0 * px * blk.exp * (9.0 * blk.cin + blk.cout),
          px * blk.cin * esize(G) + px * blk.cout * (esize(T) * (res ? 2 : 1) + (yb ? 2 : 0)) + (double)blk.exp * (9.0 * blk.cin + blk.cout) * esize(md_.act)}, s);
}

void Builder::emit_mb_head(const BlockSpec& blk, const BlockPlan& d, R dw, R part) {
    const std::string p = blk.prefix + ".block";
    const int A = md_.act, h = d.h, w = d.w;
    SymOp s = geom(FTC_OP_MBHEAD, h, w, d.ho, d.wo, blk.cin, blk.exp, 3, 1);
    ftc_op& o = s.o;
    o.act = FTC_ACT_SILU; o.in_dtype = A; o.out_dtype = A; o.w_dtype = A;
    o.Cout_total = d.mb_slice; o.aux0 = blk.squeeze; o.aux1 = d.band_rows;
    o.flags = (in_blocked_ ? FTC_FLAG_KBLOCK32 : 0) | md_.split | (d.presplit ? FTC_FLAG_PRESPLIT : 0);
    // (fp16x3: the head streams the PRE-SPLIT copy of its input)
    s.in = md_.x3 ? xb_ : gin(); s.out = dw; s.w2 = wref(p + ".0.w"); s.bias2 = wref(p + ".0.b"); s.w = wref(p + ".1.w"); s.bias = wref(p + ".1.b");
    s.scale = wref(p + ".2.w1"); s.out2 = part;
    s.aux = scratch(s, OPD_AUX);                             // the per-band channel sums: written, read by nothing
    emit({p + ".0+1", "conv1x1+dw3x3", 2.0 * B * h * w * blk.exp * (blk.cin + 9),
          (double)B * h * w * (blk.cin + blk.exp) * esize(A) + (double)blk.exp * blk.cin * esize(A) + blk.exp * 44.0 + 4.0 * blk.exp * blk.squeeze}, s);
}

void Builder::emit_mb_expand_dw(const BlockSpec& blk, const BlockPlan& d, R dw, R part) {
    const std::string p = blk.prefix + ".block";
    const int A = md_.act, h = d.h, w = d.w, ho = d.ho, wo = d.wo;
    const R e = buf((int64_t)B * h * w * blk.exp, A);
    conv(p + ".0", gin(), md_.gemm_in, h, w, blk.cin, blk.cin, 0, p + ".0", blk.exp, 1, 1, FTC_ACT_SILU, e, A);
    SymOp s = geom(FTC_OP_DWCONV, h, w, ho, wo, blk.exp, blk.exp, 3, blk.stride);
    ftc_op& o = s.o;
    o.act = FTC_ACT_SILU; o.in_dtype = A; o.out_dtype = A; o.aux0 = d.P;
    s.in = e; s.out = dw; s.w = wref(p + ".1.w"); s.bias = wref(p + ".1.b"); s.aux = part;
    emit({p + ".1", "dwconv3x3", 2.0 * B * ho * wo * blk.exp * 9, (double)B * ((double)h * w + (double)ho * wo) * blk.exp * esize(A) + blk.exp * 40.0}, s);
}

// SqueezeExcitation + project convolution of an MBConv block: dw = the depthwise output, part = the partial sums of its head
void Builder::emit_se_project(const BlockSpec& blk, const BlockPlan& d, R dw, R part, R y, const ConvOpt& tail) {
    const std::string p = blk.prefix + ".block";
    const int A = md_.act, ho = d.ho, wo = d.wo;
    const bool slice = d.form == BlockForm::MB_SLICED, foldse = d.foldse;
    const int fdt = md_.dual ? A : FTC_F32;
    SymOp s = geom(FTC_OP_SE, ho, wo, 0, 0, blk.exp, blk.exp);
    ftc_op& o = s.o;
    o.flags = (foldse ? FTC_FLAG_SE_FOLD | (md_.dual ? 0 : FTC_FLAG_SPLIT16) : 0) | (slice ? FTC_FLAG_SE_HPART : 0); o.w_dtype = foldse ? fdt : 0;
    o.Cout_total = foldse ? blk.cout : 0; o.aux0 = blk.squeeze; o.aux1 = d.P;
    const R sc = buf((int64_t)B * blk.exp, FTC_F32);
    const R hid = scratch(s, OPD_IN2);                       // the hidden layer
    const R wb = foldse ? buf((int64_t)B * blk.cout * blk.exp, fdt) : R();
    s.aux = part; s.out = sc; s.in2 = hid; s.w = wref(p + ".2.w1"); s.w2 = wref(p + ".2.w2t"); s.bias = wref(p + ".2.b1");
    s.bias2 = wref(p + ".2.b2"); s.in = foldse ? wref(p + ".3.w") : R(); s.out2 = wb;
    const double se_bytes = (slice ? 4.0 : 8.0) * blk.exp * blk.squeeze + (double)B * d.P * (slice ? blk.squeeze : blk.exp) * 4 +
                            (foldse ? (double)(B + 1) * blk.cout * blk.exp * esize(fdt) : 0.0);
    emit({p + ".2", "se", 4.0 * B * blk.exp * blk.squeeze, se_bytes}, s);
    ConvOpt pj = tail;
    pj.se = foldse ? R() : sc;
    pj.wsets = wb;
    if (d.presplit) pj.extra_flags |= FTC_FLAG_PRESPLIT;      // d was written pre-split by the fused head
    conv(p + ".3", dw, A, ho, wo, blk.exp, blk.exp, 0, p + ".3", blk.cout, 1, 1, FTC_ACT_NONE, y, Mode::trunk, pj);
}

void Builder::emit_last_1x1(int clast, int nfeat) {
    const std::string hp = "backbone.features." + std::to_string(nfeat);
    const R x4 = buf((int64_t)B * h_ * w_ * LAST_CHANNEL, md_.act);
    conv(hp, gin(), md_.gemm_in, h_, w_, clast, clast, 0, hp, LAST_CHANNEL, 1, 1, FTC_ACT_SILU, x4, md_.act);
    taps_.push_back({x4, LAST_CHANNEL, h_, w_, md_.act});
}

// One FPN level of all heads: the backbone tap it joins, the stacked tensor of the level before it, and how the convolution gets its input
struct Builder::Level {
    int i;                       // level 1.. (level 0 is the merged convolution)
    Tap tp;                      // the backbone tap of this level
    bool last;
    int cin;                     // FPN_DIM + tp.c
    int64_t M, wsz;              // pixels of the level's map (all images); bytes of one head's weights
    R y; int yh, yw;             // stacked output [9][B,yh,yw,FPN_DIM] of the level before
    bool up_in = false;          // the convolution upsamples y while it stages its halo (FTC_FLAG_UPCAT_IN): no concatenated input
    bool bn_fold = false;        // ... and reads the ONE shared copy of the tap: its BatchNorm is folded into weights `lf` + a border bias table
    std::string lf;
    R tapbn, cat;                // the batch-normed tap(s) | the materialised upsample + concat
    double src_bytes = 0;        // bytes one group's convolution reads as input
};

// Chooses the input form of level lv and emits the op that prepares it, if any
void Builder::level_input(Level& lv) {
    const int A = md_.act, nh = NHEADS, i = lv.i, tc = lv.tp.c, th = lv.tp.h, tw = lv.tp.w, tdt = lv.tp.dt, cy = FPN_DIM;
    const int ti = (int)taps_.size() - 1 - i;
    const std::string bi = std::to_string(ti);
    const R bn_s = wref("heads.in_bn." + bi + ".scale"), bn_t = wref("heads.in_bn." + bi + ".shift");
    // (round 3: also in the fp32 / fp16x3 plans, whose last-level concatenated input is 2.7 GB: FTC_NO_UPFUSE32=1 materialises it)
    const bool fuse_up = (md_.dual || !opt_.no_upfuse32) && !opt_.no_upfuse;
    // 16-bit modes, levels whose upsampled source is a stacked tensor (2..): the concatenated input is never materialised -- the
    // convolution upsamples while it stages its halo (FTC_FLAG_UPCAT_IN).  (measured: with 32-channel K blocks the per-block
    // upsampling work outweighs the saved pass, so Cin 288 keeps the two-kernel form)
    // (fp32 / fp16x3 plans: the halo kernel's K block is 32 channels of 4 bytes, and the three-MFMA product makes the upsampling work per block
    // a smaller share: level 2 -- 192 + 96 channels -- goes too; FTC_NO_UPFUSE32_L2=1: as before)
    const int kblk = (md_.dual || opt_.no_upfuse32_l2) ? 64 : 32;
    lv.up_in = fuse_up && i >= 2 && th == 2 * lv.yh && tw == 2 * lv.yw && cy % kblk == 0 && tc % kblk == 0;
    // ... and on the last level the tap's BatchNorm is folded into the weights + a border bias table, so that all heads read the ONE
    // 16-bit trunk copy of the tap  (fp32 / fp16x3 plans: the tap itself -- fp32 NHWC, what the halo loader reads)
    const R tap_copy = !md_.dual ? ((tdt == A && !opt_.no_bnfold32) ? lv.tp.buf : R()) : ti < (int)tap_copies_.size() ? tap_copies_[ti] : R();
    lv.lf = "heads.L" + std::to_string(i) + "f";
    lv.bn_fold = lv.up_in && lv.last && tap_copy && has_w(lv.lf + ".w") && !opt_.no_bnfold;
    if (lv.bn_fold) {
        lv.tapbn = tap_copy;
        lv.src_bytes = (double)B * lv.yh * lv.yw * cy * esize(A) + (double)lv.M * tc * esize(A) / nh;
    } else if (lv.up_in) {
        lv.tapbn = buf((int64_t)nh * lv.M * tc, A);
        SymOp s = geom(FTC_OP_UPCAT, th, tw, th, tw, tc, tc);
        ftc_op& o = s.o;
        o.in_dtype = A; o.out_dtype = A; o.res_dtype = tdt; o.aux0 = 0; o.aux1 = tc; o.groups = nh;
        s.in2 = lv.tp.buf; s.out = lv.tapbn; s.scale = bn_s; s.shift = bn_t;
        emit({"heads.tapbn" + std::to_string(i), "upcat", 0.0, (double)nh * lv.M * tc * esize(A) + (double)lv.M * tc * esize(tdt)}, s);
        lv.src_bytes = (double)B * lv.yh * lv.yw * cy * esize(A) + (double)lv.M * tc * esize(A);
    } else {
        const int cin = lv.cin;
        lv.cat = buf((int64_t)nh * lv.M * cin, A);
        SymOp s = geom(FTC_OP_UPCAT, lv.yh, lv.yw, th, tw, cin, cin);
        ftc_op& o = s.o;
        o.flags = i == 1 ? FTC_FLAG_GROUP_IN_SLICE : 0; o.in_dtype = A; o.out_dtype = A; o.res_dtype = tdt;
        o.Cin_total = i == 1 ? nh * FPN_DIM : FPN_DIM; o.cin_off = 0; o.aux0 = cy; o.aux1 = tc; o.groups = nh;
        s.in = lv.y; s.in2 = lv.tp.buf; s.out = lv.cat; s.scale = bn_s; s.shift = bn_t;
        emit({"heads.cat" + std::to_string(i), "upcat", 0.0,
              (double)nh * ((double)lv.M * ((double)cin * esize(A) + (double)tc * esize(tdt)) + (double)B * lv.yh * lv.yw * cy * esize(A))}, s);
        lv.src_bytes = (double)lv.M * cin * 2;
    }
}

// The 3x3 convolution of groups [g0, g0+ng) of level lv; `top`: fused top convolution (out = the tap tensor) instead of the 192-channel output
void Builder::level_conv(const Level& lv, const std::string& name, int g0, int ng, R outr, bool top) {
    const int A = md_.act, wdt = md_.act, cy = FPN_DIM, cin = lv.cin, tc = lv.tp.c, th = lv.tp.h, tw = lv.tp.w;
    const int64_t M = lv.M;
    const std::string wname = lv.bn_fold ? lv.lf : "heads.L" + std::to_string(lv.i);
    const int brows = lv.bn_fold ? 16 : 1;
    SymOp s = geom(FTC_OP_CONV, th, tw, th, tw, cin, FPN_DIM, 3, 1);
    ftc_op& o = s.o;
    o.act = FTC_ACT_GELU; o.in_dtype = A; o.out_dtype = A; o.w_dtype = wdt; o.Cout_total = FPN_DIM; o.groups = ng > 1 ? ng : 0;
    s.out = outr;
    s.w = wref(wname + ".w", (int64_t)g0 * lv.wsz);
    s.bias = wref(wname + ".b", (int64_t)g0 * brows * FPN_DIM * 4);
    int flags = md_.split;
    // weights-through-L1 kernel for the fused last level (fragment-major copy of the folded weights); FTC_NO_WL1=1: the LDS-ring halo kernel
    const bool wl1 = lv.bn_fold && has_w(lv.lf + ".wfrag") && !opt_.no_wl1;
    if (lv.bn_fold) {
        flags |= FTC_FLAG_UPCAT_IN | FTC_FLAG_BORDER_BIAS | FTC_FLAG_GROUP_IN2_SHARED;
        o.Cin_total = cy; o.aux0 = 65;
        s.in = sub(lv.y, (int64_t)g0 * B * lv.yh * lv.yw * cy * esize(A)); s.in2 = lv.tapbn;
        if (wl1) { flags |= FTC_FLAG_W_FRAG; s.w = wref(lv.lf + ".wfrag", (int64_t)g0 * lv.wsz); }
    } else if (lv.up_in) {
        flags |= FTC_FLAG_UPCAT_IN;
        o.Cin_total = cy; o.aux0 = 65;
        s.in = sub(lv.y, (int64_t)g0 * B * lv.yh * lv.yw * cy * esize(A)); s.in2 = sub(lv.tapbn, (int64_t)g0 * M * tc * esize(A));
    } else {
        o.Cin_total = cin;
        s.in = sub(lv.cat, (int64_t)g0 * M * cin * esize(A));
    }
    double flops = 2.0 * ng * M * FPN_DIM * cin * 9;
    double byt = ng * (lv.src_bytes + (double)FPN_DIM * cin * 9 * esize(wdt));
    if (top) {
        flags |= FTC_FLAG_TOP_FUSE;
        int nout = 0;
        for (int g = 0; g < NMAP; ++g) nout += HEADS[g].out_dim;
        o.aux0 = 65; o.aux1 = TW;
        s.w2 = wref("heads.top8.wt");
        flops += 2.0 * M * FPN_DIM * 9 * nout;
        byt += (double)ng * M * TW * 4;
    } else {
        byt += (double)ng * M * FPN_DIM * esize(A);
    }
    o.flags = flags;
    if (wl1) o.aux0 |= 128;
    emit({name, "conv3x3", flops, byt}, s);
}

// The nine heads.  Level 0 of all of them is one convolution (see pack_weights); levels 1.. are ONE grouped launch each (upsample+concat,
// then the 3x3 convolution) over head-major stacked tensors [9][B,h,w,C].
void Builder::emit_heads() {
    const int A = md_.act, nh = NHEADS, ntap = (int)taps_.size();
    const Tap t4 = taps_[ntap - 1];
    const R y0 = buf((int64_t)B * t4.h * t4.w * nh * FPN_DIM, A);
    {
        ConvOpt c;
        c.extra_flags = FTC_FLAG_BORDER_BIAS;
        conv("heads.upsamplers.0", t4.buf, t4.dt, t4.h, t4.w, t4.c, t4.c, 0, "heads.L0", nh * FPN_DIM, 3, 1, FTC_ACT_GELU, y0, A, c);
    }
    R y = y0;
    int yh = t4.h, yw = t4.w;
    // (round 5: in the fp32 / fp16x3 plans too -- fp32 FMA epilogue, conv_epilogue_topfuse_f32; FTC_NO_TOPFUSE32=1: the two-kernel form)
    const bool fuse_top = (md_.dual || !opt_.no_topfuse32) && taps_[0].c + FPN_DIM == 256 && !opt_.no_topfuse;
    for (int i = 1; i < ntap; ++i) {
        Level lv{i, taps_[ntap - 1 - i], i == ntap - 1};
        lv.cin = FPN_DIM + lv.tp.c;
        lv.M = (int64_t)B * lv.tp.h * lv.tp.w;
        lv.wsz = (int64_t)FPN_DIM * lv.cin * 9 * esize(md_.act);
        lv.y = y; lv.yh = yh; lv.yw = yw;
        level_input(lv);
        const int64_t M = lv.M;
        if (lv.last && fuse_top) {
            // Last level: the eight map heads never store their 192-channel output -- the epilogue multiplies the tile by the head's
            // top-convolution taps and stores 20 floats per pixel; TAPSUM does the 9-point sum into the heat-map channels.  The feature
            // head (100 output channels) keeps the two-kernel form.
            const R Tt = buf((int64_t)NMAP * M * TW, FTC_F32);
            int nout = 0;
            for (int g = 0; g < NMAP; ++g) nout += HEADS[g].out_dim;
            level_conv(lv, "heads.upsamplers." + std::to_string(i) + "+top", 0, NMAP, Tt, true);
            SymOp s = geom(FTC_OP_TAPSUM, lv.tp.h, lv.tp.w, lv.tp.h, lv.tp.w);
            s.o.Cout_total = 10; s.o.aux0 = TW; s.o.aux1 = nout; s.o.groups = NMAP;
            s.in = Tt; s.out = HEATMAP; s.w = wref("heads.top8.map"); s.bias = wref("heads.top8.b");
            emit({"heads.top8.tapsum", "tapsum", 0.0, (double)NMAP * M * TW * 4 + (double)M * nout * 4}, s);
            const R yf = buf(M * FPN_DIM, A);
            level_conv(lv, "feature.upsamplers." + std::to_string(i), nh - 1, 1, yf, false);
            ConvOpt c;
            c.cout_total = FEATURE_DIM;
            conv("feature.top_conv", yf, A, lv.tp.h, lv.tp.w, FPN_DIM, FPN_DIM, 0, "feature.top_conv", FEATURE_DIM, 3, 1, FTC_ACT_NONE, FEATURES, FTC_F32, c);
            return;
        }
        const R ynew = buf((int64_t)nh * M * FPN_DIM, A);
        level_conv(lv, "heads.upsamplers." + std::to_string(i), 0, nh, ynew, false);
        y = ynew;
        yh = lv.tp.h; yw = lv.tp.w;
    }
    emit_top_convs(y, yh, yw);
}

// The top convolutions as launches of their own, on the stacked last-level tensor y
void Builder::emit_top_convs(R y, int yh, int yw) {
    const int A = md_.act;
    const int64_t gs = (int64_t)B * yh * yw * FPN_DIM * esize(A);          // bytes between the heads' last-level tensors
    for (int hi = 0; hi < NHEADS; ++hi) {
        const R yi = sub(y, hi * gs);
        const std::string name = HEADS[hi].name;
        ConvOpt c;
        if (hi >= 2 && hi < 8) {
            if (hi != 2) continue;                                       // covered by the grouped launch
            c.cout_total = 10; c.cout_off = HEADS[hi].ch0 + 1; c.groups = 6; c.extra_flags = FTC_FLAG_GROUP_OUT_SLICE;
            conv("heads.top6", yi, A, yh, yw, FPN_DIM, FPN_DIM, 0, "heads.top6", 1, 3, 1, FTC_ACT_NONE, HEATMAP, FTC_F32, c);
        } else if (HEADS[hi].ch0 >= 0) {                                 // map heads write straight into their channel slice; channel 1 is the NMS slot
            c.cout_total = 10; c.cout_off = HEADS[hi].ch0 == 0 ? 0 : HEADS[hi].ch0 + 1;
            conv(name + ".top_conv", yi, A, yh, yw, FPN_DIM, FPN_DIM, 0, name + ".top_conv", HEADS[hi].out_dim, 3, 1, FTC_ACT_NONE, HEATMAP, FTC_F32, c);
        } else {
            c.cout_total = FEATURE_DIM;
            conv(name + ".top_conv", yi, A, yh, yw, FPN_DIM, FPN_DIM, 0, name + ".top_conv", HEADS[hi].out_dim, 3, 1, FTC_ACT_NONE, FEATURES, FTC_F32, c);
        }
    }
}

void Builder::emit_nms(int mh, int mw) {
    SymOp s = geom(FTC_OP_NMS, mh, mw, mh, mw);
    s.o.Cout_total = 10;
    s.out = HEATMAP;
    emit({"nms", "nms", 0.0, (double)B * mh * mw * 8.0}, s);
}

int Builder::build(ModelPlan* out) {
    const auto stages = backbone_blocks(m_->size);
    emit_stem(stage_rows(m_->size)[0].cin);
    // every block's form, decided once and from the last block to the first: a block's output layout follows what the next block reads
    std::vector<const BlockSpec*> flat;
    for (const auto& st : stages)
        for (const BlockSpec& blk : st) flat.push_back(&blk);
    std::vector<BlockPlan> plan(flat.size());
    {
        std::vector<std::pair<int, int>> in(flat.size());
        int h = h_, w = w_;
        for (size_t i = 0; i < flat.size(); ++i) { in[i] = {h, w}; h = (h - 1) / flat[i]->stride + 1; w = (w - 1) / flat[i]->stride + 1; }
        for (size_t i = flat.size(); i-- > 0;)
            plan[i] = decide_block(*flat[i], in[i].first, in[i].second, i > 0 || md_.dual, i + 1 < flat.size() ? &plan[i + 1] : nullptr);
    }
    size_t bi = 0;
    for (size_t si = 0; si < stages.size(); ++si) {
        for (const BlockSpec& blk : stages[si]) emit_block(blk, plan[bi++]);
        if (si + 1 == 2 || si + 1 == 3 || si + 1 == 5) {          // BackboneModel.forward taps (models/detector.py:143)
            taps_.push_back({x_, stages[si].back().cout, h_, w_, Mode::trunk});
            tap_copies_.push_back(xb_);
        }
    }
    emit_last_1x1(stages.back().back().cout, (int)stages.size() + 1);
    const int mh = taps_[0].h, mw = taps_[0].w;
    emit_heads();
    emit_nms(mh, mw);
    if (!err_.empty()) return ftc_set_error(FTC_ERR_INVALID, "ftc model plan: " + err_);
    return finish(out, mh, mw);
}

// SimpleDecoder.forward (models/detector.py:249-254) on `H` gathered feature rows: ops 3i .. 3i+2 = head i; the head's output is
// addressed through FTC_BASE_HEATMAP so that ftc_decoder_forward runs each op range with that base pointing at its own buffer.
int Builder::build_decoder(ModelPlan* out) {
    const int A = md_.act;
    for (int i = 0; i < 3; ++i) {
        const std::string q = "decoder." + std::to_string(i), name = "decoder.blocks." + std::to_string(i);
        const R a = buf((int64_t)H * DECODER_MID, A), b = buf((int64_t)H * DECODER_MID, A);
        conv(name + ".0", IMAGE, A, H, 1, DECODER_KPAD, DECODER_KPAD, 0, q + ".l0", DECODER_MID, 1, 1, FTC_ACT_GELU, a, A);
        conv(name + ".3", a, A, H, 1, DECODER_MID, DECODER_MID, 0, q + ".l1", DECODER_MID, 1, 1, FTC_ACT_GELU, b, A);
        conv(name + ".6", b, A, H, 1, DECODER_MID, DECODER_MID, 0, q + ".l2", DECODER_MODULO[i], 1, 1, FTC_ACT_NONE, HEATMAP, FTC_F32);
    }
    if (!err_.empty()) return ftc_set_error(FTC_ERR_INVALID, "ftc decoder plan: " + err_);
    return finish(out, H, 1);
}

// liveness-based first-fit arena + resolution of the symbolic operands
int Builder::finish(ModelPlan* out, int mh, int mw) {
    if (opt_.shrink_buf >= 0 && opt_.shrink_buf < (int)bufs_.size()) bufs_[opt_.shrink_buf].nbytes -= ALIGN;      // (tests: the fit check below must refuse it)
    // The arena places buffers side by side: an operand that runs past the buffer reserved for it would run into a live neighbour
    for (size_t i = 0; i < ops_.size(); ++i) {
        OpExtents e;
        if (op_extents(form_of(ops_[i]), &e) != nullptr) continue;                       // (a refused form: plan validation reports it)
        for (int j = 0; j < FTC_NUM_OPERANDS; ++j) {
            const R& r = (&ops_[i].in)[j];
            if (r.kind != 1 || e.state[j] == FTC_OPERAND_UNUSED || r.extra + e.bytes[j] <= bufs_[r.v].nbytes) continue;
            return ftc_set_error(FTC_ERR_INVALID, "ftc model plan: op " + std::to_string(i) + " (" + meta_[i].name + "): operand " + kOperandName[j] + " spans " +
                                                      std::to_string(e.bytes[j]) + " bytes from offset " + std::to_string(r.extra) + " of a buffer of " +
                                                      std::to_string(bufs_[r.v].nbytes));
        }
    }
    std::vector<int> order(bufs_.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bufs_[a].first < bufs_[b].first; });
    struct Iv { int64_t off, end; int last; };
    std::vector<Iv> live;
    int64_t top = 0, peak = 0;
    for (int bi : order) {
        Buf& b = bufs_[bi];
        if (b.last < 0) return ftc_set_error(FTC_ERR_INVALID, "ftc model plan: buffer never used");
        live.erase(std::remove_if(live.begin(), live.end(), [&](const Iv& iv) { return iv.last < b.first; }), live.end());
        std::sort(live.begin(), live.end(), [](const Iv& a, const Iv& c) { return a.off < c.off || (a.off == c.off && a.end < c.end); });
        int64_t off = 0;
        for (const Iv& iv : live) {
            if (off + b.nbytes <= iv.off) break;
            off = std::max(off, iv.end);
        }
        b.offset = off;
        live.push_back({off, off + b.nbytes, b.last});
        top = std::max(top, off + b.nbytes);
        int64_t sum = 0;
        for (const Iv& iv : live) sum += iv.end - iv.off;
        peak = std::max(peak, sum);
    }
    auto res = [&](const R& r) -> ftc_ref {
        ftc_ref f{};
        switch (r.kind) {
        case 1: f.base = FTC_BASE_WORKSPACE; f.offset = bufs_[r.v].offset + r.extra; break;
        case 2: f.base = FTC_BASE_WEIGHTS; f.offset = r.v; break;
        case 3: f.base = FTC_BASE_INPUT; break;
        case 4: f.base = FTC_BASE_HEATMAP; break;
        case 5: f.base = FTC_BASE_FEATURES; break;
        default: break;
        }
        return f;
    };
    out->plan.ops.clear();
    for (const SymOp& s : ops_) {
        ftc_op o = s.o;
        o.in = res(s.in); o.in2 = res(s.in2); o.out = res(s.out); o.w = res(s.w); o.w2 = res(s.w2); o.bias = res(s.bias); o.bias2 = res(s.bias2);
        o.scale = res(s.scale); o.shift = res(s.shift); o.aux = res(s.aux); o.out2 = res(s.out2);
        out->plan.ops.push_back(o);
    }
    apply_tuning(out->plan.ops.data(), (int)out->plan.ops.size(), opt_);             // measured kernel choice per conv shape (ftc_op.aux0)
    out->plan.workspace_bytes = align_up(top);
    out->plan.weights_bytes = (int64_t)m_->blob.bytes.size();
    out->meta = meta_;
    out->B = B; out->H = H; out->W = W; out->h = mh; out->w = mw;
    out->peak_live_bytes = peak;
    out->total_buffer_bytes = 0;
    for (const Buf& b : bufs_) out->total_buffer_bytes += b.nbytes;
    return FTC_OK;
}

}  // namespace

int build_model_plan(ftc_model* m, int B, int H, int W, bool nchw, const PlanOptions& opt, ModelPlan* out) { return Builder(m, B, H, W, nchw, opt).build(out); }

int build_decoder_plan(ftc_model* m, int rows, const PlanOptions& opt, ModelPlan* out) { return Builder(m, 1, rows, 1, false, opt).build_decoder(out); }

}  // namespace ftc_model_detail

extern "C" {

int ftc_conv_signature(const ftc_op* op, char* buf, int len) {
    if (!op || !buf) return ftc_set_error(FTC_ERR_INVALID, "ftc_conv_signature: null arguments");
    if (op->kind != FTC_OP_CONV) return ftc_set_error(FTC_ERR_INVALID, "ftc_conv_signature: not an FTC_OP_CONV");
    const std::string sig = ftc_model_detail::conv_signature(*op);
    if (len <= (int)sig.size()) return ftc_set_error(FTC_ERR_INVALID, "ftc_conv_signature: buffer too short for " + sig);
    std::memcpy(buf, sig.c_str(), sig.size() + 1);
    return FTC_OK;
}

int ftc_tune_ops(ftc_op* ops, int n_ops) {
    if (!ops || n_ops < 0) return ftc_set_error(FTC_ERR_INVALID, "ftc_tune_ops: null / negative arguments");
    return ftc_model_detail::apply_tuning(ops, n_ops, ftc_model_detail::read_plan_options());
}

}  // extern "C"
