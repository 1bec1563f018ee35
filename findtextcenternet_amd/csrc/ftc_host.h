// Host-side definitions shared by the C-ABI translation units (ftc_api.hip; pack.hip, plan.hip and model.hip through model_net.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ftc.h"
#include "backbone_choice.h"
#include "conv_choice.h"
#include "op_extents.h"
#include "wgrad_choice.h"

struct ftc_plan {
    std::vector<ftc_op> ops;
    int64_t workspace_bytes;
    int64_t weights_bytes;
};

// Records the thread-local message returned by ftc_last_error() and returns `code`.
int ftc_set_error(int code, const std::string& msg);

// backbone_choice.h: the kernel choice of FTC_OP_STEM, DWCONV, SE, MBHEAD, FMBCONV and UPCAT (backbone::<kind>_resolve + <kind>_format_label) and the geometry
// the plan builder asks before it emits an op (ftc_mbhead_legal, ftc_mbhead_band_rows, ftc_mbhead_bands, ftc_mbhead_slice, ftc_fmbconv_legal, ...)

// conv_choice.h: the choice of a convolution op, conv_validate (NULL if the op, incl. its tuned kernel choice ftc_op.aux0, is supported, else the reason)
// and conv_pinned_choice / conv_small_tile_choice, which write a choice back into aux0

// op_extents.h: op_extents -- per operand of an op whether its form uses it and the bytes it spans, or the reason the form is refused

// wgrad.hip: the kernel label of an FTC_OP_WGRAD op (wgrad_choice.h: wgrad_resolve + wgrad_format_label)
void wgrad_kernel_label(const ftc_op& op, char* buf, int len);

// ftc_api.hip: opt-in of `kernel` to `bytes` (> 64 KB) of dynamic LDS, made once per (kernel, device): looks up the calling thread's
// current device, so it holds when that changes and when host threads race on a first launch; afterwards its only HIP call is hipGetDevice.
hipError_t ftc_allow_dyn_lds(const void* kernel, int bytes);
// ftc_api.hip: compute units of the current device (asked once per device)
hipError_t ftc_device_cus(int* n_cu);

// page_merge.hip: the header block in the scratch of the rank-ordered page selections (ftc_page_merge; ftc_page_fill in page_fill.hip) and the two
// of its kernels both use -- the exclusive prefix sum of the neighbour counts (more edges than `cap`: use_seq = 1) and the kept ranks -> keep_idx
struct PmHdr { int n_keep, ticket, use_seq, big_lock, total_edges, stall_r, stall_j, stall_n; };      // stall_*: the first wait that ran into the spin limit
hipError_t launch_pm_scan(int* cnt, int* cursor, int N, long cap, PmHdr* hdr, hipStream_t s);
hipError_t launch_pm_compact(const int* status, const int* order, int N, int* keep_idx, PmHdr* hdr, hipStream_t s);
// page_merge.hip: the tail of both selections -- separator filter (seps > sep_th; NaN: none) and 3x3 code maxima behind a keep list
hipError_t launch_page_finish(const float* loc, const int* keep_idx, const int* n_keep, const float* seps, const float* codes, int mh, int mw, int scale,
                              double sep_th, float* out_loc, int* out_idx, int* out_n, hipStream_t s);

// glyph_select.hip: the per-glyph code-point selection kernel behind ftc_glyph_select / ftc_glyph_decode (arguments validated by the caller)
hipError_t ftc_glyph_select_launch(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int n,
                                   float* s0, float* s1, float* s2, int64_t* ids, float* probs, hipStream_t stream);
