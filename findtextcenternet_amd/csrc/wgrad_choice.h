// The kernel choice of FTC_OP_WGRAD, made in ONE place: wgrad_resolve() turns an ftc_op (its fields, flags and the split count in aux0) into a
// WgradChoice or the reason the op is refused.  validate_op (plan creation), ftc_op_kernel_label (what tests, tools and bench.py read) and
// launch_wgrad (what runs) all consume that one result, so a label is by construction the formatted form of the launch.
// Host only: ftc.h and the standard library, no HIP header and no kernel -- a plain C++ program can include it.
//
// Two bits of ftc_op.flags force a kernel (A/B measurements, tests that reach a kernel its successor has taken the shapes of):
//   WGRAD_FORCE_GENERIC (0x100)  the generic kernel, whatever the shape;
//   WGRAD_FORCE_STAGED  (0x200)  the register-staged form in place of a transpose-read one: wgrad3_kernel for wgrad3t_kernel, the generic kernel for
//                                the DMA ring.
// Accepted but not honoured (tests/golden/wgrad_choices.json.gz pins today's behaviour):
//   * either bit on an op the generic kernel takes anyway, and WGRAD_FORCE_STAGED on an op of the thin kernel, which has no other form;
//   * every other flag but FTC_FLAG_SE_SCALE (and FTC_FLAG_SIDE_STREAM, which the plan runner reads): no kernel looks at them.
#pragma once
#include <cstdio>

#include "../../include/ftc.h"

namespace wgradimpl {

enum { WGRAD_FORCE_GENERIC = 0x100, WGRAD_FORCE_STAGED = 0x200 };

// The five kernel families, in the one order wgrad_resolve tests them.
enum WgradFamily { WGRAD_THIN, WGRAD_NINE_TR, WGRAD_NINE_STAGED, WGRAD_RING, WGRAD_GENERIC };

// Tiles of the generic kernel (output channels x input channels per workgroup); the launcher maps the index to wgrad_kernel's template arguments.
struct WgTile { int BM, BN; const char* name; };
static const WgTile kWgTile[] = {{32, 128, "32x128"}, {64, 64, "64x64"}, {128, 128, "128x128"}, {192, 256, "192x256"}};
enum { WG_TILE_32x128 = 0, WG_TILE_64x64, WG_TILE_128x128, WG_TILE_192x256 };

struct WgradChoice {
    int family;                     // WgradFamily
    int tile;                       // generic: WG_TILE_*, else -1
    int w_dtype, x_dtype, dz_dtype; // compute type; storage of the layer input and of the output gradient
    int thin_co, thin_ks;           // thin: output channels (1 | 2) and ksize (1 | 3), else 0
    int bk;                         // pixels per K step (0: the thin kernel has none)
    long chunk;                     // pixels per split
    bool gated, se_epi;             // an SE gate; applied to the partial tile's columns instead of every staged element
    int nseg;                       // nine-tap kernels: 32-pixel segments per image row ...
    long steps_per_split;           // ... and (image, segment, row) steps per split
    int splits;
    unsigned grid[3];
    int lds_bytes;                  // dynamic LDS of the launch
    int KK;                         // taps the reduction sums
    bool reduce_wide;               // wgrad_reduce_wide_kernel follows instead of wgrad_reduce_kernel
};

inline bool is16(int dt) { return dt == FTC_BF16 || dt == FTC_F16; }

inline bool wgrad_thin_shape(int Cout, int Cin, int ksize, int stride) { return Cout <= 2 && stride == 1 && (ksize == 3 || ksize == 1) && Cin % 8 == 0 && Cin <= 1024; }

inline bool wgrad3_shape(int Wo, int Cout, int Cin, int ksize) { return ksize == 3 && Wo % 32 == 0 && Cout >= 32 && Cin >= 32; }

inline int wgrad_tile(int Cout, int Cin, int ksize) {
    if (Cout <= 32) return WG_TILE_32x128;
    if (Cout <= 64 || Cin <= 64) return WG_TILE_64x64;
    // every (Cout tile, Cin tile, tap) workgroup re-reads its two operand streams: the kernel is bound by those re-reads (last FPN level:
    // 4.7 GB per launch at 128 x 128), so wide layers take the 192 x 256 tile (12 accumulators per wave, one workgroup per CU)
    if (ksize == 3 && Cout >= 192 && Cin >= 256) return WG_TILE_192x256;        // (1x1 layers: measured slower, 25.5 -> 29.6 ms per step)
    return WG_TILE_128x128;
}

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

// Pixel splits a layer should ask for (ftc_wgrad_splits; the caller passes them back in ftc_op.aux0).  Built from the resolver's shape predicates and
// tile table, but with no dtype, stride, slice or flag to go by, so it APPROXIMATES the choice: a 3x3 layer with Wo % 32 == 0 gets the nine-tap kernels'
// tile count even where the generic kernel runs (fp32 compute, fp32 operand storage, stride 2, a gated input), a layer of thin shape the thin
// kernel's rule even where its output gradient is a 16-bit copy, and the 192 x 256 tile is counted where mixed storage falls back to 128 x 128.
// These values are the project's measured behaviour (tests/golden/wgrad_choices.json.gz, part "splits") and stay.
inline int wgrad_splits(int B, int Ho, int Wo, int Cout, int Cin, int ksize) {
    const WgTile& t = kWgTile[wgrad_tile(Cout, Cin, ksize)];
    long tiles = ceil_div(Cout, t.BM) * ceil_div(Cin, t.BN) * ksize * ksize;
    if (wgrad3_shape(Wo, Cout, Cin, ksize)) tiles = ceil_div(Cout, 64) * ceil_div(Cin, 64);      // the nine-tap kernels: 64 x 64 tiles, taps inside
    const long P = (long)B * Ho * Wo;
    if (wgrad_thin_shape(Cout, Cin, ksize, 1)) {                  // (the thin kernel: one workgroup per ~1024 pixels, at most 512)
        const long st = ceil_div(P, 1024);
        return (int)(st < 1 ? 1 : st > 512 ? 512 : st);
    }
    long S = ceil_div(1536, tiles);                               // ~6 workgroups per CU in flight
    // ... but every split writes (and the reduction re-reads) a full fp32 copy of the gradient: on the deep stages (4608 pixels, 1.5 M
    // weights) 16 splits moved 200 MB of partial sums around 33 MB of operands.  At least 1024 pixels (16 K steps) per split.
    const long smax = ceil_div(P, 1024);
    if (S > smax) S = smax;
    if (S < 1) S = 1;
    if (S > 4096) S = 4096;
    return (int)S;
}

// The choice `o` runs with and NULL, or the reason the op is refused (the choice is then not filled).  What is checked here is the op's form; the extents of
// its buffers are op_extents.h's.
inline const char* wgrad_resolve(const ftc_op& o, WgradChoice* choice) {
    if (o.Cin <= 0 || o.Cout <= 0 || o.Ho <= 0 || o.Wo <= 0 || (o.ksize != 1 && o.ksize != 3) || (o.stride != 1 && o.stride != 2)) return "wgrad: bad sizes";
    if (o.w_dtype != FTC_F32 && !is16(o.w_dtype)) return "wgrad: unknown compute type";
    if ((o.in_dtype != FTC_F32 && o.in_dtype != o.w_dtype) || (o.res_dtype != FTC_F32 && o.res_dtype != o.w_dtype))
        return "wgrad: operands are fp32 or 16-bit copies in the compute type (in_dtype: layer input, res_dtype: output gradient)";
    const int pad = (o.ksize - 1) / 2;
    if (o.Ho != (o.H + 2 * pad - o.ksize) / o.stride + 1 || o.Wo != (o.W + 2 * pad - o.ksize) / o.stride + 1) return "wgrad: Ho/Wo inconsistent";
    const int CinT = o.Cin_total > 0 ? o.Cin_total : o.Cin, CoutT = o.Cout_total > 0 ? o.Cout_total : o.Cout;
    if ((long)o.cin_off + o.Cin > CinT || (long)o.cout_off + o.Cout > CoutT || o.aux0 < 1 || o.aux0 > 4096) return "wgrad: channel slices / splits out of range";

    WgradChoice& c = *choice;
    const int S = o.aux0, KK = o.ksize * o.ksize;
    const long P = (long)o.B * o.Ho * o.Wo, HoWo = (long)o.Ho * o.Wo;
    const int BK = o.w_dtype == FTC_F32 ? 32 : 64;
    const bool generic = (o.flags & WGRAD_FORCE_GENERIC) != 0, staged = (o.flags & WGRAD_FORCE_STAGED) != 0;
    // both operands are 16-bit copies in the compute type / every channel count, stride and offset is a whole 16-byte access of them
    const bool copies16 = is16(o.w_dtype) && o.in_dtype == o.w_dtype && o.res_dtype == o.w_dtype;
    const bool al8 = o.Cout % 8 == 0 && o.Cin % 8 == 0 && CoutT % 8 == 0 && CinT % 8 == 0 && o.cout_off % 8 == 0 && o.cin_off % 8 == 0;
    c.tile = -1; c.w_dtype = o.w_dtype; c.x_dtype = o.in_dtype; c.dz_dtype = o.res_dtype; c.thin_co = c.thin_ks = 0;
    c.bk = BK; c.chunk = ceil_div(ceil_div(P, S), BK) * BK;
    c.gated = (o.flags & FTC_FLAG_SE_SCALE) != 0;
    c.se_epi = c.gated && o.ksize == 1 && o.stride == 1 && c.chunk > 0 && HoWo % c.chunk == 0;         // every split lies inside one image
    c.nseg = 0; c.steps_per_split = 0; c.splits = S; c.lds_bytes = 0; c.KK = KK; c.reduce_wide = S >= 48;
    c.grid[0] = c.grid[1] = 1; c.grid[2] = S;
    if (wgrad_thin_shape(o.Cout, o.Cin, o.ksize, o.stride) && o.res_dtype == FTC_F32 && !c.gated && o.H == o.Ho && o.W == o.Wo && !generic && CinT % 8 == 0 &&
        o.cin_off % 8 == 0) {
        c.family = WGRAD_THIN; c.thin_co = o.Cout; c.thin_ks = o.ksize; c.bk = 0; c.chunk = ceil_div(P, S);
        c.grid[0] = S; c.grid[2] = 1;
        return nullptr;
    }
    if (wgrad3_shape(o.Wo, o.Cout, o.Cin, o.ksize) && o.stride == 1 && copies16 && !c.gated && !generic) {
        c.family = al8 && !staged ? WGRAD_NINE_TR : WGRAD_NINE_STAGED; c.bk = 32;
        c.nseg = o.Wo / 32;
        c.steps_per_split = ceil_div((long)o.B * c.nseg * o.Ho, S);
        c.grid[0] = (unsigned)ceil_div(o.Cout, 64); c.grid[1] = (unsigned)ceil_div(o.Cin, 64);
        return nullptr;
    }
    // 1x1 stride 1, no per-element gate, buffer addressing in 32 bits: the DMA ring
    if (o.ksize == 1 && o.stride == 1 && copies16 && (!c.gated || c.se_epi) && !generic && !staged && al8 && o.Cout >= 64 && o.Cin >= 64 &&
        P * CoutT * 2 < 0x7fffffffL && P * CinT * 2 < 0x7fffffffL && c.chunk % 32 == 0) {
        c.family = WGRAD_RING; c.bk = 32;
        c.grid[0] = (unsigned)ceil_div(o.Cout, 128); c.grid[1] = (unsigned)ceil_div(o.Cin, 128);
        c.lds_bytes = 4 * 32 * 256 * 2;                              // four stages of 32 pixels x (128 + 128) channels
        return nullptr;
    }
    c.family = WGRAD_GENERIC;
    c.tile = wgrad_tile(o.Cout, o.Cin, o.ksize);
    // the 192 x 256 tile has one staging task per thread only with 16-byte accesses of 8 channels (16-bit copies) or the fp32 K step of 32
    if (c.tile == WG_TILE_192x256 && is16(o.w_dtype) && !copies16) c.tile = WG_TILE_128x128;
    c.grid[0] = (unsigned)ceil_div(o.Cout, kWgTile[c.tile].BM); c.grid[1] = (unsigned)(ceil_div(o.Cin, kWgTile[c.tile].BN) * KK);
    return nullptr;
}

// The kernel label (ftc_op_kernel_label) of an op running with choice `c`: the kernel template as a profiler shows it, every argument that selects an
// instantiation, the form of the SE gate where the kernel has one, and the reduction kernel that follows.
inline void wgrad_format_label(const ftc_op&, const WgradChoice& c, char* buf, int len) {
    const char* dt[] = {"f32", "bf16", "f16", "?"};
    const char* gate = !c.gated ? "" : c.se_epi ? ",gate=epi" : ",gate=staged";
    const char* red = c.reduce_wide ? "+reduce_wide" : "+reduce";
    switch (c.family) {
    case WGRAD_THIN: snprintf(buf, len, "wgrad_thin_kernel<x=%s,co=%d,k=%d>%s", dt[c.x_dtype & 3], c.thin_co, c.thin_ks, red); return;
    case WGRAD_NINE_TR: snprintf(buf, len, "wgrad3t_kernel<%s>%s", dt[c.w_dtype & 3], red); return;
    case WGRAD_NINE_STAGED: snprintf(buf, len, "wgrad3_kernel<%s>%s", dt[c.w_dtype & 3], red); return;
    case WGRAD_RING: snprintf(buf, len, "wgrad1t_kernel<%s%s>%s", dt[c.w_dtype & 3], gate, red); return;
    default:
        snprintf(buf, len, "wgrad_kernel<%s,x=%s,dz=%s,tile=%s,bk=%d%s>%s", dt[c.w_dtype & 3], dt[c.x_dtype & 3], dt[c.dz_dtype & 3], kWgTile[c.tile & 3].name, c.bk, gate, red);
    }
}

}  // namespace wgradimpl
