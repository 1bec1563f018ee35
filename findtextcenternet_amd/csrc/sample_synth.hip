// include/ftc_sample.h: the reference's training-sample synthesis (dataset/processer.pyx: the affine crop, the Gaussian centre map, the
// log-size box maps, the id maps, the text-line / separator rasters and the colour composition) for a batch of samples described by a
// device table.  The definition the kernels implement -- every rounding and every float64 promotion of the reference's generated C++ --
// is written out in the header; tests/sample_oracle.py restates it in NumPy and tests/golden/g18_sample_synth.npz pins both against
// the reference's own outputs.
//
// Four launches on the caller's stream: init (centre 0, boxes +inf, ids 0, minsize +inf) -> glyph scatter (one workgroup per glyph;
// max / min through global atomics on order-preserving integer images of the floats, so any order gives the same bits) -> maps (rasters
// into channels 3, 4; decodes the boxes, inf -> 0; decodes minsize) and, independent of those, the image (resample + composition fused).
// Compiled with -ffp-contract=off (build.py); the pragma below says the same for a reader of this file alone.
#include <cmath>
#include <cstdint>
#include <string>

#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_sample.h"
#include "../../include/ftc_sample_aug.h"

#pragma clang fp contract(off)

static_assert(sizeof(ftc_sample_desc) == 280, "ftc_sample_desc is a fixed 280-byte record (mirrored in _lib.py)");

namespace {

constexpr unsigned SS_INF_BITS = 0x7f800000u;

// order-preserving image of a float in the unsigned integers (no NaN comes here), and back
__device__ __forceinline__ unsigned ss_enc(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ss_dec(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// (int) of a float as x86 does it where the value fits; beyond +-2^30 clamped (such a coordinate is far outside every page and map, and
// stays outside after the +1 / +-2 the callers add), NaN -> the low clamp
__device__ __forceinline__ int ss_int(float v) {
    if (!(v > -1073741824.f)) return -1073741824;
    if (v > 1073741824.f) return 1073741824;
    return (int)v;
}
__device__ __forceinline__ int ss_int(double v) {
    if (!(v > -1073741824.0)) return -1073741824;
    if (v > 1073741824.0) return 1073741824;
    return (int)v;
}

// vector_dot of the reference: v = 0; v += a[0] * x; v += a[1] * y; v += a[2] * 1
__device__ __forceinline__ void ss_dot(const float* a, float x, float y, float& ox, float& oy) {
    float v = 0.f;
    v += a[0] * x;
    v += a[1] * y;
    v += a[2] * 1.f;
    ox = v;
    v = 0.f;
    v += a[3] * x;
    v += a[4] * y;
    v += a[5] * 1.f;
    oy = v;
}

struct SsWeights { float w11, w21, w12, w22; int X, Y; };

// header P1: three of the four weights are float64 products rounded once to fp32
__device__ __forceinline__ SsWeights ss_weights(float rx, float ry) {
    const float dx = rx - floorf(rx), dy = ry - floorf(ry);
    SsWeights w;
    w.w11 = (float)((1.0 - (double)dx) * (1.0 - (double)dy));
    w.w21 = (float)((double)dx * (1.0 - (double)dy));
    w.w12 = (float)((1.0 - (double)dx) * (double)dy);
    w.w22 = dx * dy;
    w.X = ss_int(rx);
    w.Y = ss_int(ry);
    return w;
}

__device__ __forceinline__ float ss_bilinear(const SsWeights& w, float p11, float p21, float p12, float p22) {
    float v = w.w11 * p11;
    v += w.w21 * p21;
    v += w.w12 * p12;
    v += w.w22 * p22;
    return v;
}

// getpixel / getpixelclip on a one-channel uint8 raster
template <bool CLIP>
__device__ __forceinline__ float ss_raster(const uint8_t* im, int h, int w, int x, int y) {
    if (x < 0 || x >= w || y < 0 || y >= h) return 0.f;
    const unsigned v = im[(size_t)y * w + x];
    if (CLIP && v <= 30u) return 0.f;
    return (float)v / 255.f;
}

// getpixel on the gray page with the inverse_partial rectangle as a predicate
__device__ __forceinline__ float ss_page(const ftc_sample_desc& d, int x, int y) {
    if (x < 0 || x >= d.im_w || y < 0 || y >= d.im_h) return 0.f;
    unsigned v = d.image[(size_t)y * d.im_w + x];
    if (y >= d.inv_y0 && y < d.inv_y1 && x >= d.inv_x0 && x < d.inv_x1) v = 255u - v;
    return (float)v / 255.f;
}

__device__ __forceinline__ float ss_page_colour(const ftc_sample_desc& d, int x, int y, int c) {
    if (x < 0 || x >= d.im_w || y < 0 || y >= d.im_h) return 0.f;
    return (float)d.image[((size_t)y * d.im_w + x) * 3 + c] / 255.f;
}

// expf, correctly rounded (header, "Transcendentals"): float64 exp rounded once.  The single-precision device routine is within 1 ulp but
// returns 0 below -103.28, where the correctly rounded value is still the smallest subnormal: that would move the centre map's zero set.
__device__ __forceinline__ float ss_expf(float e) { return (float)exp((double)e); }

// header P5
__device__ __forceinline__ float ss_compose(float a, float fg, float bg) { return (float)((double)(a * fg) + (1.0 - (double)a) * (double)bg); }

__global__ __launch_bounds__(256) void ss_init_kernel(int mapn, float* __restrict__ labelmap, int* __restrict__ idmap, float* __restrict__ minsize) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) reinterpret_cast<unsigned*>(minsize)[b] = SS_INF_BITS;
    if (i >= mapn) return;
    float* lab = labelmap + (size_t)b * 5 * mapn;
    lab[i] = 0.f;
    const unsigned inf = 0xff800000u;             // ss_enc(+inf)
    reinterpret_cast<unsigned*>(lab)[mapn + i] = inf;
    reinterpret_cast<unsigned*>(lab)[2 * mapn + i] = inf;
    int* id = idmap + (size_t)b * 2 * mapn;
    id[i] = 0;
    id[mapn + i] = 0;
}

// one workgroup per (glyph, sample); every store is an atomic max / min on a cell inside [0, mh) x [0, mw)
__global__ __launch_bounds__(256) void ss_glyph_kernel(const ftc_sample_desc* __restrict__ descs, int H, int W, int s, float* __restrict__ labelmap,
                                                       int* __restrict__ idmap, float* __restrict__ minsize) {
    const int b = blockIdx.y, g = blockIdx.x;
    const ftc_sample_desc& d = descs[b];
    if ((d.flags & FTC_SAMPLE_BLANK) || g >= d.n_glyphs) return;
    const int mh = H / s, mw = W / s, mapn = mh * mw;
    const float px = d.position[g * 4 + 0], py = d.position[g * 4 + 1], pw = d.position[g * 4 + 2], ph = d.position[g * 4 + 3];
    float xr1, yr1, xr2, yr2;
    ss_dot(d.fwd, px - pw / 2.f, py - ph / 2.f, xr1, yr1);
    ss_dot(d.fwd, px + pw / 2.f, py + ph / 2.f, xr2, yr2);
    const float cx = (xr1 + xr2) / 2.f - d.startx, cy = (yr1 + yr2) / 2.f - d.starty;
    const float gw = xr2 - xr1, gh = yr2 - yr1;
    if (!(cx > 0.f && cx < (float)W && cy > 0.f && cy < (float)H)) return;
    const float fs = (float)s;
    unsigned* lab = reinterpret_cast<unsigned*>(labelmap + (size_t)b * 5 * mapn);
    int* id = idmap + (size_t)b * 2 * mapn;

    if (threadIdx.x == 0) {
        const float m = gh > gw ? gh : gw;
        if (m > 0.f) atomicMin(reinterpret_cast<unsigned*>(minsize) + b, __float_as_uint(m));      // positive floats order as their bits
    }

    {   // centre map
        const float ccx = cx / fs, ccy = cy / fs, w4 = gw / fs, h4 = gh / fs;
        const double tw = (double)w4 / 2.0, th = (double)h4 / 2.0;
        const float fix_w = 1.0 > tw ? 1.f : (float)tw, fix_h = 1.0 > th ? 1.f : (float)th;
        const double ka = (double)fix_h * 1.5, kb = (double)fix_w * 1.5;
        const double kd = ka > kb ? ka : kb;                                                         // header P4
        const int klim = mh + mw + 2;                       // a window this wide covers the map from every centre: a larger k changes nothing
        const int k = kd < (double)klim ? ss_int(kd) : klim;
        const float sx = fix_w / 4.f, sy = fix_h / 4.f;
        const double vx = (double)(sx * sx), vy = (double)(sy * sy);
        const int xi = (int)roundf(ccx), yi = (int)roundf(ccy);      // 0 < ccx < mw: xi in [0, mw]
        const int x0 = max(0, xi - k), x1 = min(mw - 1, xi + k), y0 = max(0, yi - k), y1 = min(mh - 1, yi + k);
        const int cw = x1 - x0 + 1, ch = y1 - y0 + 1;
        if (k >= 0 && cw > 0 && ch > 0) {
            for (int t = threadIdx.x; t < cw * ch; t += 256) {
                const int x = x0 + t % cw, y = y0 + t / cw;
                const float ax = (float)(x - xi), ay = (float)(y - yi);
                const float ex = (float)(((-0.5 * (double)ax) * (double)ax) / vx);                   // header P3
                const float ey = (float)(((-0.5 * (double)ay) * (double)ay) / vy);
                const float v = ss_expf(ey) * ss_expf(ex);
                if (v == v) atomicMax(lab + y * mw + x, __float_as_uint(v));                         // v >= 0
            }
        }
    }
    {   // box maps and id maps: the same ellipse
        const double tw = (double)gw / 10.0, th = (double)gh / 10.0;
        const float bw = (double)s > tw ? fs : (float)tw, bh = (double)s > th ? fs : (float)th;
        const float sizex = (float)((double)logf(gw / 1024.f) + 3.0), sizey = (float)((double)logf(gh / 1024.f) + 3.0);
        const int c1 = d.codes[g * 2 + 0], c2 = d.codes[g * 2 + 1];
        const int x0 = max(0, ss_int((cx - bw) / fs) - 2), x1 = min(mw, ss_int((cx + bw) / fs) + 2);
        const int y0 = max(0, ss_int((cy - bh) / fs) - 2), y1 = min(mh, ss_int((cy + bh) / fs) + 2);
        const int cw = x1 - x0, ch = y1 - y0;
        if (cw > 0 && ch > 0) {
            for (int t = threadIdx.x; t < cw * ch; t += 256) {
                const int x = x0 + t % cw, y = y0 + t / cw;
                const float qx = ((float)(x * s) - cx) / bw, qy = ((float)(y * s) - cy) / bh;
                const float qx2 = qx * qx, qy2 = qy * qy;
                if (qx2 + qy2 < 1.f) {
                    const int i = y * mw + x;
                    if (sizex == sizex) atomicMin(lab + mapn + i, ss_enc(sizex));
                    if (sizey == sizey) atomicMin(lab + 2 * mapn + i, ss_enc(sizey));
                    atomicMax(id + i, c1);
                    atomicMax(id + mapn + i, c2);
                }
            }
        }
    }
}

// one thread per map cell: channels 3 and 4, the box maps decoded in place (not finite -> 0), minsize decoded by the first thread
__global__ __launch_bounds__(256) void ss_map_kernel(const ftc_sample_desc* __restrict__ descs, int H, int W, int s, float* __restrict__ labelmap,
                                                     float* __restrict__ minsize) {
    const int b = blockIdx.y;
    const int mh = H / s, mw = W / s, mapn = mh * mw;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const ftc_sample_desc& d = descs[b];
    if (i == 0) {
        const unsigned m = reinterpret_cast<unsigned*>(minsize)[b];
        minsize[b] = m == SS_INF_BITS ? 0.f : __uint_as_float(m);
    }
    if (i >= mapn) return;
    float* lab = labelmap + (size_t)b * 5 * mapn;
    for (int c = 1; c <= 2; ++c) {
        const float v = ss_dec(reinterpret_cast<unsigned*>(lab)[c * mapn + i]);
        lab[c * mapn + i] = isfinite(v) ? v : 0.f;
    }
    if (d.flags & FTC_SAMPLE_BLANK) {
        lab[3 * mapn + i] = 0.f;
        lab[4 * mapn + i] = 0.f;
        return;
    }
    const int x = i % mw, y = i / mw;
    float sx, sy;
    if (d.flags & FTC_SAMPLE_COLOUR) {
        sx = (float)x + d.startx / (float)s;
        sy = (float)y + d.starty / (float)s;
    } else {                                                                                         // header P6
        const float half = (float)(s / 2);
        sx = (float)((double)((float)x * half) + (double)d.startx / 2.0);
        sy = (float)((double)((float)y * half) + (double)d.starty / 2.0);
    }
    float rx, ry;
    ss_dot(d.inv2, sx, sy, rx, ry);
    const SsWeights w = ss_weights(rx, ry);
    float tl, sl;
    if (d.flags & FTC_SAMPLE_COLOUR) {
        tl = ss_bilinear(w, ss_raster<true>(d.textline, d.map_h, d.map_w, w.X, w.Y), ss_raster<true>(d.textline, d.map_h, d.map_w, w.X + 1, w.Y),
                         ss_raster<true>(d.textline, d.map_h, d.map_w, w.X, w.Y + 1), ss_raster<true>(d.textline, d.map_h, d.map_w, w.X + 1, w.Y + 1));
        sl = ss_bilinear(w, ss_raster<true>(d.sepline, d.map_h, d.map_w, w.X, w.Y), ss_raster<true>(d.sepline, d.map_h, d.map_w, w.X + 1, w.Y),
                         ss_raster<true>(d.sepline, d.map_h, d.map_w, w.X, w.Y + 1), ss_raster<true>(d.sepline, d.map_h, d.map_w, w.X + 1, w.Y + 1));
    } else {
        tl = ss_bilinear(w, ss_raster<false>(d.textline, d.map_h, d.map_w, w.X, w.Y), ss_raster<false>(d.textline, d.map_h, d.map_w, w.X + 1, w.Y),
                         ss_raster<false>(d.textline, d.map_h, d.map_w, w.X, w.Y + 1), ss_raster<false>(d.textline, d.map_h, d.map_w, w.X + 1, w.Y + 1));
        sl = ss_bilinear(w, ss_raster<false>(d.sepline, d.map_h, d.map_w, w.X, w.Y), ss_raster<false>(d.sepline, d.map_h, d.map_w, w.X + 1, w.Y),
                         ss_raster<false>(d.sepline, d.map_h, d.map_w, w.X, w.Y + 1), ss_raster<false>(d.sepline, d.map_h, d.map_w, w.X + 1, w.Y + 1));
    }
    lab[3 * mapn + i] = tl;
    lab[4 * mapn + i] = sl;
}

// one thread per output pixel: resample, the salt (include/ftc_sample_aug.h; `salt` may be null), then the composition; the gray
// intermediate stays in a register
__global__ __launch_bounds__(256) void ss_image_kernel(const ftc_sample_desc* __restrict__ descs, const ftc_salt_desc* __restrict__ salt, int H, int W,
                                                       float* __restrict__ image) {
    const int b = blockIdx.y;
    const int n = H * W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ftc_sample_desc& d = descs[b];
    float* out = image + (size_t)b * 3 * n;
    const int x = i % W, y = i / W;
    const bool blank = d.flags & FTC_SAMPLE_BLANK;
    float rx = 0.f, ry = 0.f;
    if (!blank) ss_dot(d.inv, (float)x + d.startx, (float)y + d.starty, rx, ry);
    if (d.flags & FTC_SAMPLE_COLOUR) {
        if (blank) {
            out[i] = out[n + i] = out[2 * n + i] = 0.f;
            return;
        }
        const SsWeights w = ss_weights(rx, ry);
        for (int c = 0; c < 3; ++c)
            out[c * n + i] = ss_bilinear(w, ss_page_colour(d, w.X, w.Y, c), ss_page_colour(d, w.X + 1, w.Y, c), ss_page_colour(d, w.X, w.Y + 1, c),
                                         ss_page_colour(d, w.X + 1, w.Y + 1, c));
        return;
    }
    float a = 0.f;
    if (blank) {
    } else if (d.flags & FTC_SAMPLE_NEAREST) {
        a = ss_page(d, ss_int((double)rx + 0.5), ss_int((double)ry + 0.5));                          // header P2
    } else {
        const SsWeights w = ss_weights(rx, ry);
        a = ss_bilinear(w, ss_page(d, w.X, w.Y), ss_page(d, w.X + 1, w.Y), ss_page(d, w.X, w.Y + 1), ss_page(d, w.X + 1, w.Y + 1));
    }
    if (salt && salt[b].grid) {
        const ftc_salt_desc& sd = salt[b];
        const unsigned code = sd.grid[(size_t)(y / sd.step) * sd.grid_w + x / sd.step];
        a = code == 1u ? 0.f : (code == 2u ? 1.f : a);
    }
    if (d.compose == FTC_SAMPLE_BACKGROUND) {
        const int yi = y + d.bg_y0, xi = x + d.bg_x0;
        const bool in = yi >= 0 && yi < d.bg_h && xi >= 0 && xi < d.bg_w;
        for (int c = 0; c < 3; ++c) {
            const float bgv = in ? (float)d.bg_image[((size_t)yi * d.bg_w + xi) * 3 + c] / 255.f : 0.f;
            const float v = ss_compose(a, d.fg1[c], bgv);
            out[c * n + i] = v < 1.f ? (v > 0.f ? v : 0.f) : 1.f;
        }
        return;
    }
    const bool second = d.compose == FTC_SAMPLE_DOUBLE && x > d.dbl_left && x < d.dbl_right && y > d.dbl_top && y < d.dbl_bottom;
    for (int c = 0; c < 3; ++c) out[c * n + i] = ss_compose(a, second ? d.fg2[c] : d.fg1[c], d.bg[c]);
}

int ss_hip_fail(hipError_t e, const char* what) { return ftc_set_error(FTC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

int ss_bad(int b, const char* what) { return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_synth: descriptor " + std::to_string(b) + ": " + what); }

int ss_bad_salt(int b, const char* what) { return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_synth_salt: salt record " + std::to_string(b) + ": " + what); }

}  // namespace

extern "C" {

int ftc_sample_abi_version(void) { return FTC_SAMPLE_ABI_VERSION; }

int ftc_sample_synth(const ftc_sample_desc* descs_host, const ftc_sample_desc* descs_dev, int B, int H, int W, int scale, float* image, float* labelmap,
                     int32_t* idmap, float* minsize, void* stream) {
    return ftc_sample_synth_salt(descs_host, descs_dev, nullptr, nullptr, B, H, W, scale, image, labelmap, idmap, minsize, stream);
}

int ftc_sample_synth_salt(const ftc_sample_desc* descs_host, const ftc_sample_desc* descs_dev, const ftc_salt_desc* salt_host, const ftc_salt_desc* salt_dev,
                          int B, int H, int W, int scale, float* image, float* labelmap, int32_t* idmap, float* minsize, void* stream) {
    if (!descs_host || !descs_dev || !image || !labelmap || !idmap || !minsize) return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_synth: null pointer argument");
    if (B < 1 || B > 65535) return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_synth: B outside 1..65535");
    if (H < 32 || W < 32 || H % 32 || W % 32 || H > 16384 || W > 16384 || scale < 2 || scale % 2 || H % scale || W % scale)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_synth: bad sizes (H, W multiples of 32 and of scale up to 16384, scale even)");
    int max_glyphs = 0;
    for (int b = 0; b < B; ++b) {
        const ftc_sample_desc& d = descs_host[b];
        if (d.flags & ~(FTC_SAMPLE_NEAREST | FTC_SAMPLE_BLANK | FTC_SAMPLE_COLOUR)) return ss_bad(b, "unknown flags");
        if (d.compose < FTC_SAMPLE_MONO || d.compose > FTC_SAMPLE_BACKGROUND) return ss_bad(b, "unknown compose kind");
        if (d.n_glyphs < 0 || d.n_glyphs > (1 << 24)) return ss_bad(b, "n_glyphs outside 0..2^24");
        if (!(d.flags & FTC_SAMPLE_COLOUR) && d.compose == FTC_SAMPLE_BACKGROUND) {
            if (!d.bg_image) return ss_bad(b, "null background image");
            if (d.bg_h < 1 || d.bg_w < 1 || (int64_t)d.bg_h * d.bg_w * 3 >= (1ll << 31)) return ss_bad(b, "bad background size");
            if (d.bg_y0 < 0 || d.bg_x0 < 0 || d.bg_y0 > (1 << 30) || d.bg_x0 > (1 << 30)) return ss_bad(b, "bad background offset");
        }
        if (d.flags & FTC_SAMPLE_BLANK) continue;
        if (!d.image || !d.textline || !d.sepline) return ss_bad(b, "null page pointer");
        if (d.n_glyphs > 0 && (!d.position || !d.codes)) return ss_bad(b, "null glyph list");
        if (d.im_h < 1 || d.im_w < 1 || d.map_h < 1 || d.map_w < 1 || (int64_t)d.im_h * d.im_w * 3 >= (1ll << 31) || (int64_t)d.map_h * d.map_w >= (1ll << 31))
            return ss_bad(b, "bad page size");
        if (d.n_glyphs > max_glyphs) max_glyphs = d.n_glyphs;
    }
    if (!salt_host != !salt_dev) return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_synth_salt: the salt table needs its host and its device copy");
    for (int b = 0; salt_host && b < B; ++b) {
        const ftc_salt_desc& sd = salt_host[b];
        if (!sd.grid) continue;
        if (descs_host[b].flags & FTC_SAMPLE_COLOUR) return ss_bad_salt(b, "salt on a colour-variant sample");
        if (sd.step < 1) return ss_bad_salt(b, "step < 1");
        if (sd.grid_h < (H + sd.step - 1) / sd.step || sd.grid_w < (W + sd.step - 1) / sd.step) return ss_bad_salt(b, "grid smaller than ceil(H / step) x ceil(W / step)");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int mapn = (H / scale) * (W / scale);
    const dim3 map_grid((mapn + 255) / 256, B), img_grid((H * W + 255) / 256, B);
    hipLaunchKernelGGL(ss_init_kernel, map_grid, dim3(256), 0, s, mapn, labelmap, idmap, minsize);
    if (max_glyphs > 0) hipLaunchKernelGGL(ss_glyph_kernel, dim3(max_glyphs, B), dim3(256), 0, s, descs_dev, H, W, scale, labelmap, idmap, minsize);
    hipLaunchKernelGGL(ss_map_kernel, map_grid, dim3(256), 0, s, descs_dev, H, W, scale, labelmap, minsize);
    hipLaunchKernelGGL(ss_image_kernel, img_grid, dim3(256), 0, s, descs_dev, salt_dev, H, W, image);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ss_hip_fail(e, "ftc_sample_synth");
}

}  // extern "C"
