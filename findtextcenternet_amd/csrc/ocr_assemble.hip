// include/ftc_ocr.h: the recognizer's input blocks built on the device (process_ocr_base.py:230-233 for every chunk of a page at once).
//
// A pure gather: one wave64 per output row of 106 floats = 53 float2 (424 B is a multiple of 8, not of 16; a source row of 400 B is
// 16-byte aligned).  Lanes 0..49 move the feature part, lanes 50..52 write the six flag columns, lanes 53..63 idle.  No LDS, no
// atomics; the two tables are read with wave-uniform addresses.  Every table value is checked before it becomes an address.
#include <cstdint>
#include <string>

#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_ocr.h"

namespace {

constexpr int FD = FTC_OCR_FEATURE_DIM;
constexpr int ROW = FD + FTC_OCR_FLAGS;             // 106
constexpr int WAVES = 4;                            // output rows per workgroup

__global__ __launch_bounds__(64 * WAVES) void ocr_assemble_kernel(const float* __restrict__ feats, int n_glyphs, const int32_t* __restrict__ rows,
                                                                  int n_rows, const int32_t* __restrict__ chunks, int total, int L,
                                                                  float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * WAVES + (threadIdx.x >> 6);          // output row b * L + t
    if (o >= total || lane >= ROW / 2) return;
    const int b = o / L, t = o - b * L;
    const int first = chunks[2 * b], n = chunks[2 * b + 1];
    const bool feat_lane = lane < FD / 2;
    float2 v = make_float2(0.0f, 0.0f);
    if (t == 0) {
        if (feat_lane) v = make_float2(FTC_OCR_FLAG_VALUE, -FTC_OCR_FLAG_VALUE);
    } else if (t <= n) {
        const int64_t r = (int64_t)first + (t - 1);
        bool ok = r >= 0 && r < n_rows;
        int g = -1, flags = 0;
        if (ok) {
            g = rows[2 * r];
            flags = rows[2 * r + 1];
            ok = g >= -1 && g < n_glyphs;
        }
        if (!ok) {
            v = make_float2(__builtin_nanf(""), __builtin_nanf(""));
        } else if (feat_lane) {
            if (g >= 0) v = reinterpret_cast<const float2*>(feats + (int64_t)g * FD)[lane];
        } else {
            const int k = 2 * (lane - FD / 2);
            v = make_float2(FTC_OCR_FLAG_VALUE * (float)((flags >> k) & 1), FTC_OCR_FLAG_VALUE * (float)((flags >> (k + 1)) & 1));
        }
    } else if (t == n + 1) {
        v = feat_lane ? make_float2(-FTC_OCR_FLAG_VALUE, FTC_OCR_FLAG_VALUE) : make_float2(-0.0f, -0.0f);
    }
    reinterpret_cast<float2*>(out + (int64_t)o * ROW)[lane] = v;
}

}  // namespace

extern "C" {

int ftc_ocr_abi_version(void) { return FTC_OCR_ABI_VERSION; }

int ftc_ocr_assemble(const float* glyph_feats, int n_glyphs, int feature_dim, const int32_t* rows, int n_rows, const int32_t* chunks, int B, int L,
                     float* enc_input, void* stream) {
    if (feature_dim != FD) return ftc_set_error(FTC_ERR_INVALID, "ftc_ocr_assemble: feature_dim must be " + std::to_string(FD));
    if (B < 1 || B > FTC_TEXT_MAX_BATCH) return ftc_set_error(FTC_ERR_INVALID, "ftc_ocr_assemble: B must be in 1.." + std::to_string(FTC_TEXT_MAX_BATCH));
    if (L < 3 || L > FTC_TEXT_LEN) return ftc_set_error(FTC_ERR_INVALID, "ftc_ocr_assemble: L must be in 3.." + std::to_string(FTC_TEXT_LEN));
    if (n_glyphs < 0 || n_rows < 0) return ftc_set_error(FTC_ERR_INVALID, "ftc_ocr_assemble: negative table size");
    if (!rows || !chunks || !enc_input || (n_glyphs > 0 && !glyph_feats)) return ftc_set_error(FTC_ERR_INVALID, "ftc_ocr_assemble: null pointer argument");
    if (((uintptr_t)glyph_feats | (uintptr_t)enc_input) & 7) return ftc_set_error(FTC_ERR_INVALID, "ftc_ocr_assemble: glyph_feats and enc_input must be 8-byte aligned");
    const int total = B * L;
    hipLaunchKernelGGL(ocr_assemble_kernel, dim3((total + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, (hipStream_t)stream, glyph_feats, n_glyphs, rows, n_rows,
                       chunks, total, L, enc_input);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_ocr_assemble: ") + hipGetErrorString(e));
}

}  // extern "C"
