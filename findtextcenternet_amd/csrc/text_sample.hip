// include/ftc_text_sample.h: the recognizer's training batch -- the reference's gen_feature / add_noise / generage_feature walk over a
// text, the empty-text case of format_output and pad_output's codes and mask -- for B texts in one launch.  The definition the kernel
// implements is written out in the header; tests/text_sample_oracle.py restates it in NumPy and tests/golden/g24_text_sample.npz pins
// both against the reference's own class.
//
// One workgroup of 256 threads per sample, one launch for the batch.  The walk over a text is a handful of scans over at most 2048
// characters (8 per thread) and the fill that follows reads what they leave in LDS; a scan launch and a fill launch would pass the same
// per-row records through global memory and pay a second launch for 42 400 elements a sample.  Phases, a barrier between each:
//   classify   every character: newline / whitespace / marker / glyph, emphasis character or not
//   scans      exclusive prefix counts of row-producing characters (the row number) and of whitespace; the last row-producing position
//              before a character (sp = whitespace since then) and the last marker before it (ruby); suffix minima of the FFF9 / FFFA /
//              FFFB positions (the reference's find)
//   emphasis   every thread follows the find chain (uniform LDS reads) and the workgroup marks the range of each emphasised triple
//   rows       each row-producing character that the walk reaches records (character, flags, bank row) for its row
//   fill       thread per element of [400][106]: gather of the bank row, the float64 add, one rounding to fp16; then the codes
// No atomics: every LDS and global element has exactly one writer.  Compiled with -ffp-contract=off (build.py).
#include <cmath>
#include <cstdint>
#include <string>

#include "ftc_common.h"
#include "ftc_host.h"
#include "philox_normal.h"
#include "../../include/ftc_text_sample.h"

#pragma clang fp contract(off)

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_PER = FTC_TEXT_SAMPLE_MAX_CHARS / TS_THREADS;      // characters per thread
constexpr int TS_MAXC = FTC_TEXT_SAMPLE_MAX_CHARS;
constexpr int TS_ROWS = FTC_TEXT_ROWS, TS_DIM = FTC_TEXT_FEATURE_DIM, TS_COLS = FTC_TEXT_FEATURE_DIM + FTC_TEXT_FLAG_COLS;
static_assert(TS_PER * TS_THREADS == TS_MAXC, "the characters divide among the threads");

enum : int { K_GLYPH = 0, K_NEWLINE = 1, K_SPACE = 2, K_RUBY1 = 3, K_RUBY2 = 4, K_RUBY0 = 5 };
// per-row record bits
enum : unsigned { RF_NEWLINE = 1u, RF_RUBY1 = 2u, RF_RUBY2 = 4u, RF_SP = 8u, RF_EMPH = 16u };
constexpr int ROW_NONE = -1, ROW_UNKNOWN = -2;                       // bank row of a table miss

__device__ __forceinline__ bool ts_is_space(int c) {
    return (c >= 0x9 && c <= 0xd) || c == 0x20 || c == 0x85 || c == 0xa0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200a) || c == 0x2028 ||
           c == 0x2029 || c == 0x202f || c == 0x205f || c == 0x3000;
}

__device__ __forceinline__ bool ts_is_emphasis(int c) {
    return c == 0x2022 || c == 0x25e6 || c == 0x25cf || c == 0x25cb || c == 0x25ce || c == 0x25c9 || c == 0x25b2 || c == 0x25b3 || c == 0xfe45 ||
           c == 0xfe46;
}

__device__ __forceinline__ int ts_kind(int c) {
    if (c == 0xa) return K_NEWLINE;
    if (ts_is_space(c)) return K_SPACE;
    if (c == 0xfff9) return K_RUBY1;
    if (c == 0xfffa) return K_RUBY2;
    if (c == 0xfffb) return K_RUBY0;
    return K_GLYPH;
}

struct OpAdd { __device__ static int id() { return 0; } __device__ static int f(int a, int b) { return a + b; } };
struct OpMax { __device__ static int id() { return -1; } __device__ static int f(int a, int b) { return a > b ? a : b; } };
struct OpMin { __device__ static int id() { return TS_MAXC; } __device__ static int f(int a, int b) { return a < b ? a : b; } };

// Exclusive scan of one value per thread in thread order (reverse = from the last thread down); buf holds 2 * TS_THREADS ints.
template <class Op>
__device__ int ts_block_scan(int v, int* buf, bool reverse) {
    const int t = reverse ? TS_THREADS - 1 - (int)threadIdx.x : (int)threadIdx.x;
    int* cur = buf;
    int* nxt = buf + TS_THREADS;
    __syncthreads();                                                // buf may still be read by the scan before
    cur[t] = v;
    __syncthreads();
    for (int d = 1; d < TS_THREADS; d <<= 1) {
        nxt[t] = t >= d ? Op::f(cur[t - d], cur[t]) : cur[t];
        __syncthreads();
        int* s = cur; cur = nxt; nxt = s;
    }
    return t ? cur[t - 1] : Op::id();
}

// one rounding to nearest even from float64 to fp16: float64 -> fp32 rounded to odd (exact, or truncated with the last bit set), which keeps
// 13 bits below fp16's last and a sticky bit, then the fp32 -> fp16 conversion rounds once
__device__ __forceinline__ _Float16 ts_f64_to_f16(double v) {
    float f = (float)v;
    if (v == v && !isinf(f) && (double)f != v) {
        unsigned b = __float_as_uint(f);
        if (fabs((double)f) > fabs(v)) b -= 1u;                      // back to the truncation toward zero
        f = __uint_as_float(b | 1u);
    }
    return (_Float16)f;
}

template <bool FP32>
__global__ __launch_bounds__(TS_THREADS) void ts_kernel(ftc_text_bank bank, const ftc_text_sample_desc* __restrict__ descs, const int32_t* __restrict__ chars,
                                                        void* __restrict__ feature, int64_t* __restrict__ in_codes, int64_t* __restrict__ out_codes) {
    __shared__ unsigned char kind[TS_MAXC];
    __shared__ unsigned char emph[TS_MAXC];
    __shared__ short ws_before[TS_MAXC + 1];                          // whitespace characters before position i
    __shared__ short nextA[TS_MAXC + 1], nextB[TS_MAXC + 1], nextC[TS_MAXC + 1];      // first FFF9 / FFFA / FFFB at or after i (TS_MAXC: none)
    __shared__ int scan_buf[2 * TS_THREADS];
    __shared__ int row_char[TS_ROWS];                                // the character of a row, ROW_NONE for rows the walk did not write
    __shared__ int row_bank[TS_ROWS];                                // its bank row, ROW_UNKNOWN for the unknown-code path
    __shared__ unsigned row_flags[TS_ROWS];
    __shared__ int s_total_rows;

    const int b = blockIdx.x, tid = threadIdx.x;
    const ftc_text_sample_desc& d = descs[b];
    const int n = d.n_chars < 0 ? 0 : (d.n_chars > TS_MAXC ? TS_MAXC : d.n_chars);      // the host validated it; the clamp keeps LDS indices in range regardless
    const int32_t* text = chars + d.text_offset;
    const bool horizontal = d.flags & FTC_TEXT_HORIZONTAL;
    const int i0 = tid * TS_PER;

    // classify
    int c[TS_PER], k[TS_PER];
    bool any_emph_char = false;
#pragma unroll
    for (int q = 0; q < TS_PER; ++q) {
        const int i = i0 + q;
        c[q] = i < n ? text[i] : 0;
        k[q] = i < n ? ts_kind(c[q]) : K_SPACE;                       // past the end: produces no row, changes no result
        any_emph_char = any_emph_char || (i < n && ts_is_emphasis(c[q]));
        kind[i] = (unsigned char)k[q];
        emph[i] = 0;
    }
    for (int r = tid; r < TS_ROWS; r += TS_THREADS) row_char[r] = ROW_NONE, row_bank[r] = ROW_NONE, row_flags[r] = 0u;
    const int has_emph = __syncthreads_or(any_emph_char);

    // scans: this thread's aggregates, then the exclusive scan over the threads, then the walk through its own characters
    int prod = 0, ws = 0, last_prod = -1, last_marker = -1, fa = TS_MAXC, fb = TS_MAXC, fc = TS_MAXC;
#pragma unroll
    for (int q = 0; q < TS_PER; ++q) {
        const int i = i0 + q;
        if (k[q] <= K_NEWLINE && i < n) prod += 1, last_prod = i;
        if (k[q] == K_SPACE && i < n) ws += 1;
        if (k[q] >= K_RUBY1) last_marker = i * 4 + (k[q] == K_RUBY1 ? 1 : (k[q] == K_RUBY2 ? 2 : 0));
    }
#pragma unroll
    for (int q = TS_PER - 1; q >= 0; --q) {
        if (k[q] == K_RUBY1) fa = i0 + q;
        if (k[q] == K_RUBY2) fb = i0 + q;
        if (k[q] == K_RUBY0) fc = i0 + q;
    }
    int row = 1 + ts_block_scan<OpAdd>(prod, scan_buf, false);
    int wsb = ts_block_scan<OpAdd>(ws, scan_buf, false);
    int lp = ts_block_scan<OpMax>(last_prod, scan_buf, false);
    int lm = ts_block_scan<OpMax>(last_marker, scan_buf, false);
    int na = ts_block_scan<OpMin>(fa, scan_buf, true);
    int nb = ts_block_scan<OpMin>(fb, scan_buf, true);
    int nc = ts_block_scan<OpMin>(fc, scan_buf, true);
    if (tid == TS_THREADS - 1) {
        s_total_rows = row - 1 + prod;
        nextA[TS_MAXC] = nextB[TS_MAXC] = nextC[TS_MAXC] = (short)TS_MAXC;
    }
#pragma unroll
    for (int q = TS_PER - 1; q >= 0; --q) {
        const int i = i0 + q;
        if (k[q] == K_RUBY1) na = i;
        if (k[q] == K_RUBY2) nb = i;
        if (k[q] == K_RUBY0) nc = i;
        nextA[i] = (short)na, nextB[i] = (short)nb, nextC[i] = (short)nc;
    }
    int my_row[TS_PER], my_lp[TS_PER], my_ruby[TS_PER];
#pragma unroll
    for (int q = 0; q < TS_PER; ++q) {
        const int i = i0 + q;
        ws_before[i] = (short)wsb;
        my_row[q] = row, my_lp[q] = lp, my_ruby[q] = lm < 0 ? 0 : (lm & 3);
        if (i < n) {
            if (k[q] <= K_NEWLINE) row += 1, lp = i;
            if (k[q] == K_SPACE) wsb += 1;
            if (k[q] >= K_RUBY1) lm = i * 4 + (k[q] == K_RUBY1 ? 1 : (k[q] == K_RUBY2 ? 2 : 0));
        }
    }
    if (tid == TS_THREADS - 1) ws_before[TS_MAXC] = (short)wsb;
    __syncthreads();

    // emphasis: the find chain, followed by every thread alike; the ranges of two triples never overlap
    if (has_emph) {
        int a = nextA[0];
        while (a < n) {
            const int m = nextB[a];
            if (m >= n) break;
            const int e = nextC[m];
            if (e >= n) break;
            if (ts_is_emphasis(text[m + 1]))                          // m + 1 <= e < n
                for (int i = a + 1 + tid; i < e; i += TS_THREADS) emph[i] = 1;
            a = nextA[e];
        }
    }
    __syncthreads();

    // rows: one record per row the walk writes
#pragma unroll
    for (int q = 0; q < TS_PER; ++q) {
        const int i = i0 + q;
        if (i >= n || k[q] > K_NEWLINE || my_row[q] >= TS_ROWS) continue;
        const int r = my_row[q];
        row_char[r] = i;
        if (k[q] == K_NEWLINE) {
            row_flags[r] = RF_NEWLINE;
            continue;
        }
        const bool sp = ws_before[i] - ws_before[my_lp[q] + 1] > 0;   // whitespace since the last row (my_lp = -1: since the start)
        row_flags[r] = (my_ruby[q] == 1 ? RF_RUBY1 : 0u) | (my_ruby[q] == 2 ? RF_RUBY2 : 0u) | (sp ? RF_SP : 0u) | (emph[i] ? RF_EMPH : 0u);
        int lo = 0, hi = bank.n_codes - 1, bank_row = ROW_UNKNOWN;
        while (lo <= hi) {
            const int mid = (lo + hi) >> 1;
            const int code = bank.table[mid].code;
            if (code == c[q]) {
                const ftc_text_bank_entry en = bank.table[mid];
                const int off = horizontal ? en.hori_offset : en.vert_offset, cnt = horizontal ? en.hori_count : en.vert_count;
                if (cnt > 0) {
                    unsigned pick;
                    if (d.pick) {
                        pick = (unsigned)d.pick[i];
                    } else {
                        unsigned w[4];
                        sd_philox(d.seed_pick, (uint64_t)(i >> 2), w);
                        pick = w[i & 3];
                    }
                    bank_row = off + (int)(pick % (unsigned)cnt);
                }
                break;
            }
            if (code < c[q]) lo = mid + 1; else hi = mid - 1;
        }
        row_bank[r] = bank_row;
    }
    __syncthreads();

    // fill
    const int total_rows = s_total_rows < TS_ROWS - 1 ? s_total_rows : TS_ROWS - 1;      // rows 1 .. total_rows are written by the walk
    const int eot_row = total_rows + 1;                               // == TS_ROWS: no EOT
    const double ratio = d.noise_ratio;
    const size_t fbase = (size_t)b * TS_ROWS * TS_COLS;
    for (int e = tid; e < TS_ROWS * TS_COLS; e += TS_THREADS) {
        const int r = e / TS_COLS, j = e - r * TS_COLS;
        _Float16 v = (_Float16)0.f;
        if (r == 0) {
            if (j < TS_DIM) v = (j & 1) ? (_Float16)-5.f : (_Float16)5.f;
        } else if (r == eot_row) {
            v = j < TS_DIM ? ((j & 1) ? (_Float16)5.f : (_Float16)-5.f) : (_Float16)-0.f;
        } else if (r <= total_rows) {
            const unsigned fl = row_flags[r];
            if (j >= TS_DIM) {
                const int col = j - TS_DIM;
                const bool on = col == 0 ? !horizontal
                              : col == 1 ? (fl & RF_RUBY1)
                              : col == 2 ? (fl & RF_RUBY2)
                              : col == 3 ? (fl & RF_SP)
                              : col == 4 ? (fl & RF_EMPH)
                                         : (fl & RF_NEWLINE);
                if (on) v = (_Float16)5.f;
            } else if (!(fl & RF_NEWLINE)) {
                const int idx = r * TS_DIM + j, br = row_bank[r];
                double base;
                if (br >= 0) {
                    _Float16 h;
                    const uint16_t bits = bank.rows[(size_t)br * TS_DIM + j];
                    __builtin_memcpy(&h, &bits, 2);
                    base = (double)h;
                } else {
                    const double z = d.z ? d.z[idx] : (double)sd_normal(d.seed_z, (uint64_t)idx);
                    base = 5.0 * z;
                }
                const double nz = d.n ? d.n[idx] : (double)sd_normal(d.seed_n, (uint64_t)idx);
                const double t10 = 10.0 * nz;
                const double noise = t10 * ratio;
                v = ts_f64_to_f16(base + noise);
            }
        }
        if (FP32) static_cast<float*>(feature)[fbase + e] = (float)v;
        else static_cast<_Float16*>(feature)[fbase + e] = v;
    }

    // codes
    const double p = d.p;
    for (int t = tid; t < FTC_TEXT_CODES; t += TS_THREADS) {
        int64_t code = FTC_TEXT_PAD;
        if (t == 0) code = FTC_TEXT_SOT;
        else if (t <= n) code = (int64_t)text[t - 1];
        else if (t == n + 1) code = FTC_TEXT_EOT;
        double u;
        if (d.u) {
            u = d.u[t];
        } else {
            unsigned w[4];
            sd_philox(d.seed_u, (uint64_t)(t >> 1), w);
            const int q = 2 * (t & 1);
            u = (double)(((uint64_t)(w[q] >> 5) << 26) | (uint64_t)(w[q + 1] >> 6)) * 0x1p-53;
        }
        out_codes[(size_t)b * FTC_TEXT_CODES + t] = code;
        in_codes[(size_t)b * FTC_TEXT_CODES + t] = u < p ? (int64_t)FTC_TEXT_MSK : code;
    }
}

int ts_bad(int b, const char* what) { return ftc_set_error(FTC_ERR_INVALID, "ftc_text_sample: descriptor " + std::to_string(b) + ": " + what); }

}  // namespace

extern "C" {

int ftc_text_sample_abi_version(void) { return FTC_TEXT_SAMPLE_ABI_VERSION; }

int ftc_text_bank_init(ftc_text_bank* bank, const uint16_t* rows_dev, const ftc_text_bank_entry* table_host, const ftc_text_bank_entry* table_dev, int n_codes,
                       int n_rows) {
    if (bank) bank->valid = 0;
    if (!bank || !rows_dev || !table_host || !table_dev) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_bank_init: null pointer argument");
    if (n_codes < 1 || n_rows < 1) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_bank_init: n_codes and n_rows must be at least 1");
    for (int i = 0; i < n_codes; ++i) {
        const ftc_text_bank_entry& e = table_host[i];
        const std::string at = "ftc_text_bank_init: entry " + std::to_string(i) + ": ";
        if (e.code < 0) return ftc_set_error(FTC_ERR_INVALID, at + "negative code");
        if (i && e.code <= table_host[i - 1].code) return ftc_set_error(FTC_ERR_INVALID, at + "codes are not strictly ascending");
        if (e.hori_offset < 0 || e.hori_count < 0 || e.vert_offset < 0 || e.vert_count < 0) return ftc_set_error(FTC_ERR_INVALID, at + "negative offset or count");
        if ((int64_t)e.hori_offset + e.hori_count > n_rows || (int64_t)e.vert_offset + e.vert_count > n_rows)
            return ftc_set_error(FTC_ERR_INVALID, at + "offset + count exceeds the bank's " + std::to_string(n_rows) + " rows");
    }
    bank->rows = rows_dev, bank->table = table_dev, bank->n_rows = n_rows, bank->n_codes = n_codes, bank->reserved = 0;
    bank->valid = FTC_TEXT_BANK_VALID;
    return FTC_OK;
}

int ftc_text_sample(const ftc_text_bank* bank, const ftc_text_sample_desc* descs_host, const ftc_text_sample_desc* descs_dev, int B, const int32_t* chars,
                    int64_t total_chars, void* feature, int feature_fp32, int64_t* in_codes, int64_t* out_codes, void* stream) {
    if (!bank || !descs_host || !descs_dev || !feature || !in_codes || !out_codes) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_sample: null pointer argument");
    if (bank->valid != FTC_TEXT_BANK_VALID || !bank->rows || !bank->table || bank->n_codes < 1 || bank->n_rows < 1)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_sample: the bank was not validated by ftc_text_bank_init");
    if (B < 1 || B > 65536) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_sample: B outside 1..65536");
    if (total_chars < 0 || (total_chars > 0 && !chars)) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_sample: bad chars / total_chars");
    for (int b = 0; b < B; ++b) {
        const ftc_text_sample_desc& d = descs_host[b];
        if (d.n_chars < 0) return ts_bad(b, "negative text length");
        if (d.n_chars > FTC_TEXT_SAMPLE_MAX_CHARS) return ts_bad(b, "text longer than FTC_TEXT_SAMPLE_MAX_CHARS");
        if (d.text_offset < 0 || d.text_offset > total_chars - d.n_chars) return ts_bad(b, "text outside chars");
        if (d.flags & ~FTC_TEXT_HORIZONTAL) return ts_bad(b, "unknown flags");
        if (std::isnan(d.noise_ratio) || std::isnan(d.p)) return ts_bad(b, "noise_ratio or p is NaN");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (feature_fp32)
        hipLaunchKernelGGL(ts_kernel<true>, dim3(B), dim3(TS_THREADS), 0, s, *bank, descs_dev, chars, feature, in_codes, out_codes);
    else
        hipLaunchKernelGGL(ts_kernel<false>, dim3(B), dim3(TS_THREADS), 0, s, *bank, descs_dev, chars, feature, in_codes, out_codes);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_text_sample: ") + hipGetErrorString(e));
}

}  // extern "C"
