// include/ftc_prep.h: the "fill selection" of the reference's data-preparation programs (the annotation pre-labeller's and the feature
// sampler's eval(): a page-sized ownership map instead of the pairwise coverage rule of page_merge.hip, a pixel-count ink rule, other
// constants) and the gather of glyph features at given centres.  The definition the kernels implement is written out in the header;
// tests/fill_oracle.py restates it in NumPy and tests/golden/g17_fill_select.npz pins both against the reference's own outputs.
//
// Everything that decides is integer arithmetic (pixel sums and counts: exact in any order) or IEEE float64 / float32 with contraction
// off, so the results are bit-identical to NumPy's.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_prep.h"

#pragma clang fp contract(off)

namespace {

// trunc of a double as Python's int() for every value a page coordinate can take; beyond +-2^31 clamped, NaN -> 0 (never an address)
__device__ __forceinline__ long pf_trunc(double v) {
    if (v != v) return 0;
    if (v < -2147483648.0) return -2147483648L;
    if (v > 2147483647.0) return 2147483647L;
    return (long)v;
}

struct PfRect { int x0, y0, cw, ch; };          // columns x0 .. x0+cw-1, rows y0 .. y0+ch-1; cw = ch = 0: empty
__device__ __forceinline__ PfRect pf_rect(double cx, double cy, double w, double h, int PH, int PW) {
    const long x0 = max(0L, pf_trunc(cx - w / 2)), x1 = min((long)PW - 1, pf_trunc(cx + w / 2) + 1);
    const long y0 = max(0L, pf_trunc(cy - h / 2)), y1 = min((long)PH - 1, pf_trunc(cy + h / 2) + 1);
    if (x1 <= x0 || y1 <= y0) return {0, 0, 0, 0};
    return {(int)x0, (int)y0, (int)(x1 - x0), (int)(y1 - y0)};     // 0 <= x0 < x1 <= PW - 1: inside the page
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- step 3's count: one workgroup per row -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pf_ink_kernel(const float* __restrict__ loc, int N, const float* __restrict__ page, int PH, int PW, float cut_off,
                                                     const double* __restrict__ th5, long long* __restrict__ ink) {
    __shared__ unsigned long long s_sum[3], s_cnt;
    const int i = blockIdx.x, t = threadIdx.x;
    const double p = loc[(long)i * 9], cx = loc[(long)i * 9 + 1], cy = loc[(long)i * 9 + 2], w = loc[(long)i * 9 + 3], h = loc[(long)i * 9 + 4];
    const PfRect r = pf_rect(cx, cy, w, h, PH, PW);
    const long n = (long)r.cw * r.ch;
    if (p < (double)cut_off || n == 0) {                          // (block-uniform)
        if (t == 0) ink[i] = 0;
        return;
    }
    if (t < 3) s_sum[t] = 0ull;
    if (t == 3) s_cnt = 0ull;
    __syncthreads();
    unsigned long long s[3] = {0ull, 0ull, 0ull};
    for (long k = t; k < n; k += 256) {
        const float* px = page + ((long)(r.y0 + (int)(k / r.cw)) * PW + r.x0 + (int)(k % r.cw)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += (unsigned long long)(long long)px[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long v = wave_sum_u64(s[c]);
        if ((t & 63) == 0) atomicAdd(&s_sum[c], v);
    }
    __syncthreads();
    float mean[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) mean[c] = __fdiv_rn(__ull2float_rn(s_sum[c]), __ll2float_rn(n));
    const double th = *th5 * 0.5;
    unsigned long long cnt = 0ull;
    for (long k = t; k < n; k += 256) {
        const float* px = page + ((long)(r.y0 + (int)(k / r.cw)) * PW + r.x0 + (int)(k % r.cw)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) cnt += (double)fabsf(px[c] - mean[c]) > th ? 1ull : 0ull;
    }
    cnt = wave_sum_u64(cnt);
    if ((t & 63) == 0) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (t == 0) ink[i] = (long long)s_cnt;
}

// ---- the selection: one workgroup, candidates in score order, threads across the rectangle ---------------------------------------------
// Per candidate that passes the three local rules: (a) one pass over the rectangle of the ownership map counts the pixels per owner --
// a wave turns runs of equal owners into one atomicAdd on the owner's counter (ocnt, all zero between candidates) and the first add to
// a counter appends the owner to the list --, (b) the listed owners are judged, their counters cleared, (c) a kept candidate takes the
// free pixels.  The map, the counters and the list are handed from wave to wave of this ONE workgroup only: a workgroup barrier orders them.
constexpr int PF_T = 1024;

__global__ __launch_bounds__(PF_T) void pf_fill_kernel(const float* __restrict__ loc, const int* __restrict__ order, int N, const double* __restrict__ hist1,
                                                       const double* __restrict__ th5, float cut_off, const long long* __restrict__ ink, int PH, int PW,
                                                       int* map, int* ocnt, int* olist, int* keep_idx, int* n_keep, const int* use_seq) {
    __shared__ int s_n, s_drop;
    const int t = threadIdx.x, lane = t & 63;
    const int why = *use_seq;                                                          // 0: the parallel path did the page; 1: asked for; 2: it gave up half-way
    if (!why) return;
    if (why == 2) {                                                                    // its claims are in the map: start from a clean one
        for (long k = t; k < (long)PH * PW; k += PF_T) map[k] = -1;
        __syncthreads();
    }
    const double th = *th5 * 0.5;
    int nk = 0;
    for (int oi = 0; oi < N; ++oi) {
        const int i = order[oi];
        if ((unsigned)i >= (unsigned)N) { if (t == 0) *n_keep = -1; return; }          // (uniform) not a row: reported, never an address
        const double p = loc[(long)i * 9], cx = loc[(long)i * 9 + 1], cy = loc[(long)i * 9 + 2], w = loc[(long)i * 9 + 3], h = loc[(long)i * 9 + 4];
        if (p < (double)cut_off) break;
        const PfRect r = pf_rect(cx, cy, w, h, PH, PW);
        const long n = (long)r.cw * r.ch;
        if (n == 0) continue;                                                          // 0 / area < 0.1
        if (hist1[i] < th) continue;                                                   // NaN threshold: never true, as in NumPy
        const double a0 = w * h;
        if ((double)ink[i] / 3.0 / a0 < 0.1) continue;
        if (t == 0) { s_n = 0; s_drop = 0; }
        __syncthreads();
        const long npad = (n + 63) & ~63L;                                             // whole waves: the shuffles below need every lane
        for (long k = t; k < npad; k += PF_T) {
            int o = -1;
            if (k < n) o = map[(long)(r.y0 + (int)(k / r.cw)) * PW + r.x0 + (int)(k % r.cw)];
            const int before = __shfl_up(o, 1, 64);
            const bool head = lane == 0 || o != before;
            const unsigned long long heads = __ballot(head);
            if (head && o >= 0 && o < N) {
                const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
                const int len = later ? __ffsll((long long)later) : 64 - lane;          // lanes up to the next run's head
                if (atomicAdd(&ocnt[o], len) == 0) olist[atomicAdd(&s_n, 1)] = o;       // distinct owners: fewer than N
            }
        }
        __syncthreads();
        const int no = s_n;
        for (int q = t; q < no; q += PF_T) {
            const int j = olist[q];
            const double own = (double)atomicExch(&ocnt[j], 0);
            const double pcx = loc[(long)j * 9 + 1], pcy = loc[(long)j * 9 + 2], pw = loc[(long)j * 9 + 3], ph = loc[(long)j * 9 + 4];
            const double a1 = pw * ph;
            const double ix0 = fmax(cx - w / 2, pcx - pw / 2), iy0 = fmax(cy - h / 2, pcy - ph / 2);
            const double ix1 = fmin(cx + w / 2, pcx + pw / 2), iy1 = fmin(cy + h / 2, pcy + ph / 2);
            const double iv = fmax(ix1 - ix0, 0.0) * fmax(iy1 - iy0, 0.0);
            const double uni = a0 + a1 - iv;
            const double iou = uni > 0.0 ? iv / uni : 0.0;
            if (iou > 0.25 || iv > a0 * 0.95 || own > a1 * 0.95) s_drop = 1;
        }
        __syncthreads();
        if (!s_drop) {
            for (long k = t; k < n; k += PF_T) {
                int* m = map + (long)(r.y0 + (int)(k / r.cw)) * PW + r.x0 + (int)(k % r.cw);
                if (*m < 0) *m = i;
            }
            if (t == 0) keep_idx[nk] = i;
            ++nk;
        }
        __syncthreads();                                                               // the map for the next candidate; s_drop read by all
    }
    if (t == 0) *n_keep = nk;
}


// ---- the same selection, parallel (the scheme of pm_resolve_kernel in page_merge.hip) ----------------------------------------------------
// A candidate's fate depends only on the KEPT earlier candidates whose integer rectangle meets its own (only they can own a pixel of it), so:
//   pf_prep      rank-ordered rectangle table; the local rules (cut-off, empty rectangle, contrast, ink) -> status 0 (undecided) | 2 (dropped);
//   pf_pairs     2-D tiled all-pairs pass, twice: count, then (after the prefix sum) fill the lists of earlier undecided candidates
//                whose rectangle intersects;
//   pf_resolve   persistent waves draw candidates IN RANK ORDER from a ticket counter.  A wave waits until every listed neighbour is decided
//                (the lowest undecided ticket never waits, so there is progress wherever the waves land), counts for each kept neighbour the
//                pixels it owns inside the intersection of the two rectangles, applies the three rules, claims the free pixels of a kept
//                candidate and publishes 1 (kept) | 2 (dropped);
//   then the kept ranks -> keep_idx in rank order.
// The map holds RANKS here (rows in the sequential kernel); it never leaves the scratch.
// Hand-off between workgroups inside the launch: ownership is written with agent-scope atomicCAS(-1 -> rank) ("where no owner yet") and read
// with agent-scope atomic loads, which go past the per-CU L1 and the per-XCD L2; a wave drains its claims (s_waitcnt vmcnt(0)) and publishes
// its status word with an agent-scope release; a waiting wave polls relaxed and acquires once after the wait.  Spins are bounded: a wait
// that does not end, or lists that do not fit the scratch, set a device flag, and the sequential kernel launched behind redoes the page.
// The header block (ticket, flags) is page_merge.hip's PmHdr, and so are the prefix sum and the compaction kernel (ftc_host.h).
constexpr int PF_PT = 256;                  // candidates per tile of the all-pairs pass
constexpr int PF_SPIN_LIMIT = 1 << 19;      // polls a wave waits for one chunk of neighbours before it hands the page to the sequential kernel

__global__ __launch_bounds__(256) void pf_prep_kernel(const float* __restrict__ loc, const int* __restrict__ order, int N, const double* __restrict__ hist1,
                                                      const double* __restrict__ th5, float cut_off, const long long* __restrict__ ink, int PH, int PW,
                                                      int4* __restrict__ rrect, int* __restrict__ status, int* __restrict__ cnt, PmHdr* hdr, int force_seq) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0 && force_seq) atomicExch(&hdr->use_seq, 1);
    if (r > N) return;
    if (r == N) { cnt[N] = 0; return; }
    cnt[r] = 0;
    rrect[r] = make_int4(0, 0, 0, 0);
    status[r] = 2;
    const int i = order[r];
    if ((unsigned)i >= (unsigned)N) { atomicExch(&hdr->use_seq, 1); return; }          // the sequential kernel reports it
    const double p = loc[(long)i * 9], cx = loc[(long)i * 9 + 1], cy = loc[(long)i * 9 + 2], w = loc[(long)i * 9 + 3], h = loc[(long)i * 9 + 4];
    if (p < (double)cut_off) return;
    const PfRect q = pf_rect(cx, cy, w, h, PH, PW);
    if ((long)q.cw * q.ch == 0) return;
    if (hist1[i] < *th5 * 0.5) return;
    if ((double)ink[i] / 3.0 / (w * h) < 0.1) return;
    rrect[r] = make_int4(q.x0, q.y0, q.x0 + q.cw, q.y0 + q.ch);
    status[r] = 0;
}

// FILL = false: cnt[r] += neighbours of r inside tile column blockIdx.x;  FILL = true: nbr[cursor[r]++] = j
template <bool FILL>
__global__ __launch_bounds__(PF_PT) void pf_pairs_kernel(const int4* __restrict__ rrect, const int* __restrict__ status0, int N, int* cnt_or_cursor,
                                                         int* __restrict__ nbr, const PmHdr* hdr) {
    const int tj = blockIdx.x, tr = blockIdx.y;
    if (tj > tr || hdr->use_seq) return;
    __shared__ int4 sr[PF_PT];
    __shared__ int sel[PF_PT];
    const int t = threadIdx.x, j0 = tj * PF_PT, r = tr * PF_PT + t;
    {
        const int j = j0 + t;
        const bool ok = j < N;
        sr[t] = rrect[ok ? j : 0];
        sel[t] = ok && status0[j] != 2;                  // status is 0 | 2 until pf_resolve runs
    }
    __syncthreads();
    if (r >= N || status0[r] == 2) return;
    const int4 c = rrect[r];
    const int jn = min(PF_PT, r - j0);                   // only earlier ranks
    int n = 0;
    for (int k = 0; k < jn; ++k) {
        if (!sel[k] || !(sr[k].x < c.z && c.x < sr[k].z && sr[k].y < c.w && c.y < sr[k].w)) continue;
        if (FILL) nbr[atomicAdd(&cnt_or_cursor[r], 1)] = j0 + k;
        else ++n;
    }
    if (!FILL && n) atomicAdd(&cnt_or_cursor[r], n);
}

__global__ __launch_bounds__(256) void pf_resolve_kernel(const float* __restrict__ loc, const int* __restrict__ order, const int4* __restrict__ rrect, int* status,
                                                         const int* __restrict__ off, const int* __restrict__ nbr, int N, int PW, int* map, PmHdr* hdr) {
    if (hdr->use_seq) return;
    const int lane = threadIdx.x & 63;
    for (;;) {
        int r = 0;
        if (lane == 0) r = atomicAdd(&hdr->ticket, 1);
        r = __shfl(r, 0, 64);
        if (r >= N) break;
        if ((r & 63) == 0 && __hip_atomic_load(&hdr->use_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        if (status[r] == 2) continue;                                // a local rule dropped it (pf_prep); otherwise 0 until THIS wave decides it
        const int beg = off[r], end = off[r + 1];
        // wait until every neighbour is decided: their claims are in the map before their status word changes
        for (int base = beg; base < end; base += 64) {
            const int q = base + lane;
            const int j = q < end ? nbr[q] : -1;
            int st = (j >= 0 && j < r) ? 0 : 2;
            for (int polls = 0;; ++polls) {
                if (st == 0) st = __hip_atomic_load(status + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (!__ballot(st == 0)) break;
                __builtin_amdgcn_s_sleep(1);
                if (polls > PF_SPIN_LIMIT || ((polls & 1023) == 1023 && __hip_atomic_load(&hdr->use_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                    if (lane == 0) {
                        if (atomicAdd(&hdr->stall_n, 1) == 0) hdr->stall_r = r;
                        atomicExch(&hdr->use_seq, 2);
                    }
                    return;
                }
            }
        }
        if (end > beg) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int i = order[r];
        const double cx = loc[(long)i * 9 + 1], cy = loc[(long)i * 9 + 2], w = loc[(long)i * 9 + 3], h = loc[(long)i * 9 + 4];
        const double a0 = w * h;
        const int4 c = rrect[r];
        bool drop = false;
        for (int base = beg; base < end && !drop; base += 64) {
            const int q = base + lane;
            const int j = q < end ? nbr[q] : -1;
            const bool kept = j >= 0 && j < r && __hip_atomic_load(status + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1;
            unsigned long long m = __ballot(kept);
            while (m && !drop) {
                const int jj = __shfl(j, __ffsll((long long)m) - 1, 64);
                m &= m - 1;
                const int4 d = rrect[jj];
                const int ix0 = max(c.x, d.x), iy0 = max(c.y, d.y), iw = min(c.z, d.z) - ix0, ih = min(c.w, d.w) - iy0;      // > 0: the rectangles meet
                if (iw <= 0 || ih <= 0) continue;                       // (cannot happen: listed because they meet)
                long own = 0;
                for (long k = lane; k < (long)iw * ih; k += 64)
                    own += __hip_atomic_load(map + (long)(iy0 + (int)(k / iw)) * PW + ix0 + (int)(k % iw), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == jj ? 1 : 0;
                own = (long)wave_sum_u64((unsigned long long)own);
                if (own == 0) continue;                                 // owns nothing here: not consulted
                const int ji = order[jj];
                const double pcx = loc[(long)ji * 9 + 1], pcy = loc[(long)ji * 9 + 2], pw = loc[(long)ji * 9 + 3], ph = loc[(long)ji * 9 + 4];
                const double a1 = pw * ph;
                const double fx0 = fmax(cx - w / 2, pcx - pw / 2), fy0 = fmax(cy - h / 2, pcy - ph / 2);
                const double fx1 = fmin(cx + w / 2, pcx + pw / 2), fy1 = fmin(cy + h / 2, pcy + ph / 2);
                const double iv = fmax(fx1 - fx0, 0.0) * fmax(fy1 - fy0, 0.0);
                const double uni = a0 + a1 - iv;
                const double iou = uni > 0.0 ? iv / uni : 0.0;
                if (iou > 0.25 || iv > a0 * 0.95 || (double)own > a1 * 0.95) drop = true;
            }
        }
        if (!drop) {
            const int cw = c.z - c.x;
            for (long k = lane; k < (long)cw * (c.w - c.y); k += 64) atomicCAS(map + (long)(c.y + (int)(k / cw)) * PW + c.x + (int)(k % cw), -1, r);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // every lane's claims have been performed before the word says so
        if (lane == 0) __hip_atomic_store(status + r, drop ? 2 : 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- glyph features at given centres: one wave per centre -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pf_features_at_kernel(const float* __restrict__ centers, int K, const ftc_tile* __restrict__ tiles, int T, int first,
                                                             int nb, const float* __restrict__ feat, int fh, int fw, int C, int scale,
                                                             _Float16* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const float xk = centers[2 * (long)k], yk = centers[2 * (long)k + 1];
    int win = -1;
    for (int ti = lane; ti < T; ti += 64) {                                            // ascending per lane: the last claim stays
        const ftc_tile tl = tiles[ti];
        const bool cx = (float)((long)tl.offset_x + (long)tl.x_min * scale) < xk && xk < (float)((long)tl.offset_x + (long)tl.x_max * scale);
        const bool cy = (float)((long)tl.offset_y + (long)tl.y_min * scale) < yk && yk < (float)((long)tl.offset_y + (long)tl.y_max * scale);
        if (cx && cy) win = ti;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) win = max(win, __shfl_xor(win, o, 64));
    if (win < first || win >= first + nb) return;
    const ftc_tile tl = tiles[win];
    const long xi = pf_trunc((double)__fdiv_rn(xk - (float)tl.offset_x, (float)scale)), yi = pf_trunc((double)__fdiv_rn(yk - (float)tl.offset_y, (float)scale));
    if (xi < 0 || xi >= fw || yi < 0 || yi >= fh) return;                              // (a claim window outside the tile's map: bad record)
    const float* src = feat + (((long)(win - first) * fh + yi) * fw + xi) * C;
    for (int c = lane; c < C; c += 64) out[(long)k * C + c] = (_Float16)src[c];
}

struct FillScratch { int64_t hdr, keep_idx, ocnt, olist, status, cnt, cursor, rrect, map, nbr, nbr_cap, total; };
FillScratch fill_layout(int64_t n, int64_t ph, int64_t pw) {
    auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    FillScratch L{};
    int64_t o = 0;
    L.hdr = o; o += 256;
    L.keep_idx = o; o = up(o + n * 4);
    L.ocnt = o; o = up(o + n * 4);
    L.olist = o; o = up(o + n * 4);
    L.status = o; o = up(o + n * 4);
    L.cnt = o; o = up(o + (n + 1) * 4);
    L.cursor = o; o = up(o + (n + 1) * 4);
    L.rrect = o; o = up(o + n * 16);
    L.map = o; o = up(o + ph * pw * 4);
    L.nbr = o;                                                   // the neighbour lists take the rest of the block
    L.nbr_cap = n * 64 < (1 << 18) ? (1 << 18) : n * 64;         // room for 64 earlier intersecting candidates per box on average
    o = up(o + L.nbr_cap * 4);
    L.total = o;
    return L;
}

int hip_fail(hipError_t e, const char* what) { return ftc_set_error(FTC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

}  // namespace

extern "C" {

int ftc_prep_abi_version(void) { return FTC_PREP_ABI_VERSION; }

int ftc_page_ink(const float* locations, int n_boxes, const float* page, int page_h, int page_w, float cut_off, const double* threshold_dev,
                 int64_t* ink_out, void* stream) {
    if (!locations || !page || !threshold_dev || !ink_out) return ftc_set_error(FTC_ERR_INVALID, "ftc_page_ink: null pointer argument");
    if (n_boxes <= 0 || n_boxes > (1 << 20) || page_h <= 0 || page_w <= 0 || (int64_t)page_h * page_w > (1ll << 30))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_page_ink: bad sizes");
    hipLaunchKernelGGL(pf_ink_kernel, dim3(n_boxes), dim3(256), 0, static_cast<hipStream_t>(stream), locations, n_boxes, page, page_h, page_w, cut_off,
                       threshold_dev, reinterpret_cast<long long*>(ink_out));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : hip_fail(e, "ftc_page_ink");
}

int64_t ftc_page_fill_scratch_bytes(int n_boxes, int page_h, int page_w) {
    if (n_boxes < 0 || page_h <= 0 || page_w <= 0) return 0;
    return fill_layout(n_boxes, page_h, page_w).total;
}

int ftc_page_fill(const float* locations, const int32_t* order, int n_boxes, const double* hist1, const double* threshold_dev, const int64_t* ink,
                  float cut_off, double sep_threshold, const float* seps, const float* codes, int mh, int mw, int scale, int page_h, int page_w,
                  float* out_locations, int32_t* out_index, int32_t* out_count, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!out_count) return ftc_set_error(FTC_ERR_INVALID, "ftc_page_fill: null pointer argument");
    if (n_boxes < 0 || n_boxes > (1 << 20)) return ftc_set_error(FTC_ERR_INVALID, "ftc_page_fill: n_boxes outside 0..2^20");
    if (n_boxes == 0) {
        const hipError_t e0 = hipMemsetAsync(out_count, 0, sizeof(int32_t), s);
        return e0 == hipSuccess ? FTC_OK : hip_fail(e0, "ftc_page_fill");
    }
    if (!locations || !order || !hist1 || !threshold_dev || !ink || !seps || !codes || !out_locations || !out_index || !scratch)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_page_fill: null pointer argument");
    if (mh <= 0 || mw <= 0 || scale <= 0 || page_h <= 0 || page_w <= 0 || (int64_t)page_h * page_w > (1ll << 30))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_page_fill: bad sizes");
    const FillScratch lay = fill_layout(n_boxes, page_h, page_w);
    if (scratch_bytes < lay.nbr + 4096) return ftc_set_error(FTC_ERR_INVALID, "ftc_page_fill: scratch smaller than the fixed part of ftc_page_fill_scratch_bytes");
    const int64_t nbr_cap = (scratch_bytes - lay.nbr) / 4;                     // lists that do not fit: the page goes through the sequential kernel
    if ((uintptr_t)scratch & 255) return ftc_set_error(FTC_ERR_INVALID, "ftc_page_fill: scratch must be 256-byte aligned");
    char* sp = static_cast<char*>(scratch);
    PmHdr* hdr = reinterpret_cast<PmHdr*>(sp + lay.hdr);
    int* keep_idx = reinterpret_cast<int*>(sp + lay.keep_idx);
    int* status = reinterpret_cast<int*>(sp + lay.status);
    int* cnt = reinterpret_cast<int*>(sp + lay.cnt);
    int* cursor = reinterpret_cast<int*>(sp + lay.cursor);
    int* nbr = reinterpret_cast<int*>(sp + lay.nbr);
    int* map = reinterpret_cast<int*>(sp + lay.map);
    int4* rrect = reinterpret_cast<int4*>(sp + lay.rrect);
    const long long* ink64 = reinterpret_cast<const long long*>(ink);
    const char* fs_env = std::getenv("FTC_PAGE_FILL_SEQ");                    // A/B and tests: "1" = the sequential kernel alone
    const int force_seq = fs_env && fs_env[0] == '1';
    hipError_t e = hipMemsetAsync(hdr, 0, 256, s);                             // ticket, flags: zeroed every call
    if (e == hipSuccess) e = hipMemsetAsync(sp + lay.ocnt, 0, (size_t)n_boxes * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(sp + lay.map, 0xff, (size_t)page_h * page_w * 4, s);       // every pixel -1: no owner
    if (e != hipSuccess) return hip_fail(e, "ftc_page_fill");
    const int T = (n_boxes + PF_PT - 1) / PF_PT;
    hipLaunchKernelGGL(pf_prep_kernel, dim3((n_boxes + 256) / 256), dim3(256), 0, s, locations, order, n_boxes, hist1, threshold_dev, cut_off, ink64, page_h, page_w,
                       rrect, status, cnt, hdr, force_seq);
    hipLaunchKernelGGL(pf_pairs_kernel<false>, dim3(T, T), dim3(PF_PT), 0, s, rrect, status, n_boxes, cnt, nbr, hdr);
    (void)launch_pm_scan(cnt, cursor, n_boxes, (long)nbr_cap, hdr, s);              // (a failed launch is reported by the check below)
    hipLaunchKernelGGL(pf_pairs_kernel<true>, dim3(T, T), dim3(PF_PT), 0, s, rrect, status, n_boxes, cursor, nbr, hdr);
    hipLaunchKernelGGL(pf_resolve_kernel, dim3(512), dim3(256), 0, s, locations, order, rrect, status, cnt, nbr, n_boxes, page_w, map, hdr);
    hipLaunchKernelGGL(pf_fill_kernel, dim3(1), dim3(PF_T), 0, s, locations, order, n_boxes, hist1, threshold_dev, cut_off, ink64, page_h, page_w, map,
                       reinterpret_cast<int*>(sp + lay.ocnt), reinterpret_cast<int*>(sp + lay.olist), keep_idx, &hdr->n_keep, (const int*)&hdr->use_seq);
    e = launch_pm_compact(status, order, n_boxes, keep_idx, hdr, s);
    if (e != hipSuccess) return hip_fail(e, "ftc_page_fill");
    e = launch_page_finish(locations, keep_idx, &hdr->n_keep, seps, codes, mh, mw, scale, sep_threshold, out_locations, out_index, out_count, s);
    return e == hipSuccess ? FTC_OK : hip_fail(e, "ftc_page_fill");
}

int ftc_features_at(const float* centers, int n_centers, const ftc_tile* tiles, int n_tiles, int first_tile, int n_batch, const float* features, int fh,
                    int fw, int channels, int scale, void* out_f16, void* stream) {
    if (n_centers < 0 || n_tiles <= 0 || first_tile < 0 || n_batch <= 0 || (int64_t)first_tile + n_batch > n_tiles || fh <= 0 || fw <= 0 || channels <= 0 ||
        scale <= 0)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_features_at: bad sizes");
    if (n_centers == 0) return FTC_OK;
    if (!centers || !tiles || !features || !out_f16) return ftc_set_error(FTC_ERR_INVALID, "ftc_features_at: null pointer argument");
    hipLaunchKernelGGL(pf_features_at_kernel, dim3((n_centers + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), centers, n_centers, tiles, n_tiles,
                       first_tile, n_batch, features, fh, fw, channels, scale, static_cast<_Float16*>(out_f16));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : hip_fail(e, "ftc_features_at");
}

}  // extern "C"
