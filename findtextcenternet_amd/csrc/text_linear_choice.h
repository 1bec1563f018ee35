// The launch choice of the recognizer's linear layers (include/ftc_text_linear.h), made in ONE place: linear_resolve() turns the arguments of
// ftc_text_linear / ftc_text_linear_bwd into the reason the call is refused or into the LinearChoice the launcher runs -- the row chunks of the
// weight gradient, the grids, and per operand whether its base and pitch allow 16-byte reads.  ftc_text_linear_bwd_workspace_bytes reads the same
// chunk rule.  The one launcher (text_linear_impl.h) runs every LinearChoice as it stands for both operand formats, text_linear.hip and
// text_linear_f16.hip: the grids too, counted in tiles of TL_WG, which the launcher asserts is each format's tile; a loader that has no use for a
// 16-byte flag ignores it.  Host only: the standard library, no HIP header and no kernel -- a plain C++ program can include it.
#pragma once
#include <cstdint>

#include "../../include/ftc_text_linear.h"

namespace textlinear {

constexpr int TL_TILE = 128;                        // the tile the header's chunk rule counts in
constexpr int TL_WG = 64;                           // output tile of a workgroup, both ways (text_linear.hip: why not 128)
constexpr int TL_BK = 32;                           // reduction steps staged at a time
constexpr int64_t TL_MAX_ROWS = int64_t(1) << 30;  // 2^24 tiles of 256 threads: what grid.x takes
constexpr int TL_MAX_DIM = 1 << 21;                 // K, N: 32768 tiles fit grid.y
constexpr int64_t TL_MAX_SPAN = int64_t(1) << 40;   // floats an operand may span
constexpr int64_t TL_CHUNK_MIN_ROWS = 1024, TL_CHUNK_WGS = 1024;

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct LinearChunks { int64_t count, rows; };       // C and R of the header

// the header's rule: a pure function of (rows, K, N)
inline LinearChunks linear_chunks(int64_t rows, int K, int N) {
    const int64_t tiles = cdiv(N, TL_TILE) * cdiv(K, TL_TILE);
    int64_t c0 = cdiv(TL_CHUNK_WGS, tiles);
    if (c0 > cdiv(rows, TL_CHUNK_MIN_ROWS)) c0 = cdiv(rows, TL_CHUNK_MIN_ROWS);
    if (c0 > FTC_TEXT_LINEAR_MAX_CHUNKS) c0 = FTC_TEXT_LINEAR_MAX_CHUNKS;
    LinearChunks c;
    c.rows = cdiv(rows, c0);
    c.count = cdiv(rows, c.rows);
    return c;
}

inline const char* linear_dims_refused(int64_t rows, int K, int N) {
    if (rows < 1 || K < 1 || N < 1) return "rows, K and N must be at least 1";
    if (rows > TL_MAX_ROWS || K > TL_MAX_DIM || N > TL_MAX_DIM) return "rows <= 2^30, K <= 2^21 and N <= 2^21";
    return nullptr;
}

inline int64_t linear_workspace_floats(int64_t rows, int K, int N) {
    const LinearChunks c = linear_chunks(rows, K, N);
    return c.count > 1 ? c.count * ((int64_t)N * K + N) : 0;
}

// an operand of `nrows` rows of `extent` floats at pitch ld: the reason it is refused, or NULL
inline const char* linear_operand_refused(const void* p, int64_t ld, int64_t nrows, int64_t extent) {
    if (!p) return "a required pointer is NULL";
    if (ld < extent) return "a pitch is below its row's extent";
    if (ld > TL_MAX_SPAN || (nrows - 1) > (TL_MAX_SPAN - extent) / ld) return "an operand spans 2^40 floats or more";
    if ((uintptr_t)p % 4) return "a pointer is not aligned to a float";
    return nullptr;
}

// 16-byte reads of rows at pitch ld from p
inline bool linear_vec(const void* p, int64_t ld) { return (uintptr_t)p % 16 == 0 && ld % 4 == 0; }

struct LinearLaunch { unsigned grid[3]; };          // (tiles of C's rows, tiles of C's columns, chunks)

// An M x N output in `chunks` slices of the reduction.  Without a product (dbias alone) only the first column of tiles exists.
inline LinearLaunch linear_launch(int64_t M, int64_t N, int64_t chunks, bool product = true) {
    LinearLaunch l;
    l.grid[0] = (unsigned)cdiv(M, TL_WG); l.grid[1] = product ? (unsigned)cdiv(N, TL_WG) : 1; l.grid[2] = (unsigned)chunks;
    return l;
}

struct LinearChoice {
    bool vec_x, vec_w, vec_dy;          // 16-byte reads allowed (an operand the call does not read: false)
    LinearChunks chunks;                // dw / dbias
    LinearLaunch y, dx, dw;
    int64_t ws_dw, ws_dbias;            // float offsets of the per-chunk sums in the workspace (chunks.count > 1)
};

// forward: y = x w^T (+ bias)
inline const char* linear_resolve_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* y, int64_t ldy, int64_t rows, int K, int N,
                                      LinearChoice* c) {
    if (const char* r = linear_dims_refused(rows, K, N)) return r;
    if (const char* r = linear_operand_refused(x, ldx, rows, K)) return r;
    if (const char* r = linear_operand_refused(w, ldw, N, K)) return r;
    if (const char* r = linear_operand_refused(y, ldy, rows, N)) return r;
    c->vec_x = linear_vec(x, ldx); c->vec_w = linear_vec(w, ldw); c->vec_dy = false;
    c->y = linear_launch(rows, N, 1);
    return nullptr;
}

inline const char* linear_resolve_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, const float* dx, int64_t lddx,
                                      const float* dw, int64_t lddw, const float* dbias, int64_t rows, int K, int N, const void* workspace, LinearChoice* c) {
    if (const char* r = linear_dims_refused(rows, K, N)) return r;
    if (!dx && !dw && !dbias) return "no output asked for (dx, dw and dbias are all NULL)";
    if (const char* r = linear_operand_refused(dy, lddy, rows, N)) return r;
    if (dx) {
        if (const char* r = linear_operand_refused(dx, lddx, rows, K)) return r;
        if (const char* r = linear_operand_refused(w, ldw, N, K)) return r;
    }
    if (dw) {
        if (const char* r = linear_operand_refused(dw, lddw, N, K)) return r;
        if (const char* r = linear_operand_refused(x, ldx, rows, K)) return r;
    }
    if (dbias && (uintptr_t)dbias % 4) return "a pointer is not aligned to a float";
    c->chunks = linear_chunks(rows, K, N);
    if ((dw || dbias) && c->chunks.count > 1 && (!workspace || (uintptr_t)workspace % 16)) return "the workspace must be given, 16-byte aligned";
    c->vec_x = dw && linear_vec(x, ldx); c->vec_w = dx && linear_vec(w, ldw); c->vec_dy = linear_vec(dy, lddy);
    c->dx = linear_launch(rows, K, 1);
    // without dw the weight-gradient kernel still runs for dbias, over the first K tile only and with no product
    c->dw = linear_launch(N, K, c->chunks.count, dw != nullptr);
    c->ws_dw = 0; c->ws_dbias = c->chunks.count * (int64_t)N * K;
    return nullptr;
}

// The residual forms (include/ftc_text_linear_res.h): the parent's resolve, then the added operand held to the rules of every other.  It is read
// one float per lane in the store's own pattern, so it takes no part in the 16-byte choice.
inline const char* linear_resolve_fwd_res(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* res, int64_t ldres, const float* y, int64_t ldy,
                                          int64_t rows, int K, int N, LinearChoice* c) {
    if (const char* r = linear_resolve_fwd(x, ldx, w, ldw, y, ldy, rows, K, N, c)) return r;
    return linear_operand_refused(res, ldres, rows, N);
}

inline const char* linear_resolve_bwd_add(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, const float* dx, int64_t lddx,
                                          const float* dx_add, int64_t lddxa, const float* dw, int64_t lddw, const float* dbias, int64_t rows, int K, int N,
                                          const void* workspace, LinearChoice* c) {
    if (const char* r = linear_dims_refused(rows, K, N)) return r;
    if (!dx) return dx_add ? "dx_add needs dx" : "a required pointer is NULL";
    if (const char* r = linear_resolve_bwd(x, ldx, w, ldw, dy, lddy, dx, lddx, dw, lddw, dbias, rows, K, N, workspace, c)) return r;
    return linear_operand_refused(dx_add, lddxa, rows, K);
}

}  // namespace textlinear
