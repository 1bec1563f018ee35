/*
 * ftc_text_sample.h -- C ABI of the recognizer's training batch: the reference's dataset/data_transformer.py:514-604 (add_noise,
 * generage_feature, gen_feature), the empty-text case of format_output (:665-669) and pad_output (:678-687) as one batched,
 * deterministic device call that makes feature, in_codes and out_codes for B texts.  Same library as ftc.h (libftc_hip.so), same
 * conventions: 0 or a negative ftc_status, ftc_last_error for the message, caller-owned device buffers, no device allocation, no
 * synchronisation, work enqueued on the stream passed in, everything refused before anything is enqueued.  This surface has its own
 * version number.
 *
 * Outputs for B texts (FTC_TEXT_FEATURE_DIM = 100 feature columns, FTC_TEXT_FLAG_COLS = 6 flag columns, FTC_TEXT_ROWS = 400 rows,
 * FTC_TEXT_CODES = 400 codes; PAD / SOT / EOT / MSK = 0 / 1 / 2 / 3):
 *   feature   [B][400][106] fp16, or fp32 holding exactly those fp16 values (feature_fp32 != 0)
 *   in_codes  [B][400] int64        out_codes [B][400] int64
 * Every element of all three is written.  A sample's outputs are a function of its own descriptor and text only: not of B, the batch slot or
 * the launch shape.
 *
 * The bank
 * --------
 * rows: device fp16 [n_rows][100], every row of the reference's features.npz (hori_<code> / vert_<code>).  table: n_codes records sorted
 * by code, each naming the code's horizontal rows (hori_offset .. hori_offset + hori_count - 1) and its vertical ones; a count of 0 means
 * the code has no rows in that orientation.  ftc_text_bank_init validates the HOST copy of the table once (codes >= 0 and strictly
 * ascending, counts >= 0, offsets >= 0, offset + count <= n_rows) and only then marks the ftc_text_bank as valid; ftc_text_sample refuses
 * a bank that is not so marked.  The device copy must hold the same records and must not change afterwards.
 *
 * The walk (the reference's state machine), per text c[0 .. n_chars - 1] (UTF-32 code points):
 *   SOT row = (5, -5, 5, -5, ...) over columns 0..99, flag columns +0.  EOT row = the NEGATED SOT row: (-5, 5, ...) and flag columns -0
 *   (the reference writes -SP_token, so the six flags of an EOT row carry the sign bit; every other zero of the array is +0).
 *   Row 0 is SOT.  idx = 1, sp = false, ruby = 0.  For i = 0, 1, ... while idx < 400:
 *     c[i] == U+000A          row idx: column 105 = 5;  sp = false;  idx += 1
 *     c[i] other whitespace   sp = true        (U+0009 U+000B U+000C U+000D U+0020 U+0085 U+00A0 U+1680 U+2000..U+200A U+2028 U+2029
 *                                               U+202F U+205F U+3000: the reference's UNICODE_WHITESPACE_CHARACTERS)
 *     c[i] == U+FFF9 / U+FFFA / U+FFFB      ruby = 1 / 2 / 0
 *     any other c[i]          row idx: columns 0..99 = the glyph's features (below); column 101 = 5 if ruby == 1; column 102 = 5 if
 *                             ruby == 2; column 103 = 5 if sp, and sp = false; column 104 = 5 if i is emphasised;  idx += 1
 *   Every row written by the walk (newline rows included) has column 100 = 5 when the sample is vertical (FTC_TEXT_HORIZONTAL not set).
 *   After the walk row idx is EOT if idx < 400; all later rows are +0.  A text longer than the walk reaches is cut without EOT.
 *   An empty text gives SOT at row 0 and EOT at row 1 (the same rule).
 *   Emphasis: only if the text holds one of U+2022 U+25E6 U+25CF U+25CB U+25CE U+25C9 U+25B2 U+25B3 U+FE45 U+FE46.  With find(x, from)
 *   the first position >= from holding x (or none): a = find(FFF9, 0); repeat { b = find(FFFA, a), e = find(FFFB, b); stop if any of the
 *   three is none; if c[b + 1] is an emphasis character, every index i with a < i < e is emphasised; a = find(FFF9, e) }.
 *
 * A glyph's features, for the glyph of code point c written to row r (j = 0..99), all in float64, every operation rounded on its own
 * (the source is compiled with -ffp-contract=off), in this order:
 *   (offset, count) = the table's hori entry of c if the sample is horizontal, else its vert entry; the other orientation is never used
 *   count > 0:  base_j = (double)rows[offset + (uint32)pick % count][j]
 *   otherwise (count == 0, or c not in the table):  base_j = 5.0 * z[r][j]          (the reference's unknown-code path)
 *   feature_j = fp16(base_j + (10.0 * n[r][j]) * noise_ratio)
 * fp16(.) is ONE rounding to nearest even from the float64 sum (subnormals kept, overflow to infinity): what NumPy's assignment into a
 * float16 array does.  noise_ratio = 0 uses the same formula.
 *
 * The codes.  out_codes = ([SOT] + c[0 .. n_chars - 1] + [EOT] + PAD ...)[:400]: the code points of the WHOLE text, not of the part
 * the walk reached.  in_codes[t] = MSK if u[t] < p else out_codes[t], u and p float64; SOT, EOT and PAD positions are masked like any other.
 *
 * Where the draws come from.  Each of pick, n, z, u is explicit (a device array named by the descriptor) or, when its pointer is null,
 * derived from the descriptor's seed for it.  philox(seed, ctr) are the four words r[0..3] of Philox4x32-10 as in ftc_sample_aug.h
 * ("Normals": key = (seed & 0xffffffff, seed >> 32), counter = (ctr & 0xffffffff, ctr >> 32, 0, 0)).
 *   pick  explicit: int32 [n_chars], indexed by the CHARACTER index i, read as uint32.   seeded: philox(seed_pick, i / 4)[i % 4].
 *   n, z  explicit: float64 [400][100], indexed by the output row.   seeded: (double)normal(seed_n or seed_z, r * 100 + j) of
 *         ftc_sample_aug.h: exactly the fp32 values ftc_sample_normal_fill writes, widened.
 *   u     explicit: float64 [400].   seeded: with w = philox(seed_u, t / 2), q = 2 (t % 2):
 *         u[t] = (double)(((uint64)(w[q] >> 5) << 26) | (w[q + 1] >> 6)) * 2^-53        (a 53-bit integer times 2^-53: exact, in [0, 1))
 * numpy's own streams are not reproduced.
 */
#ifndef FTC_TEXT_SAMPLE_H_
#define FTC_TEXT_SAMPLE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_SAMPLE_ABI_VERSION 1

#define FTC_TEXT_FEATURE_DIM 100
#define FTC_TEXT_FLAG_COLS 6
#define FTC_TEXT_ROWS 400
#define FTC_TEXT_CODES 400
#define FTC_TEXT_PAD 0
#define FTC_TEXT_SOT 1
#define FTC_TEXT_EOT 2
#define FTC_TEXT_MSK 3

/* the longest text of one sample (characters, markers and whitespace included) */
#define FTC_TEXT_SAMPLE_MAX_CHARS 2048

/* ftc_text_sample_desc.flags */
#define FTC_TEXT_HORIZONTAL 1

#define FTC_TEXT_BANK_VALID 0x46544231 /* set by ftc_text_bank_init */

/* One code of the bank: 20 bytes. */
typedef struct ftc_text_bank_entry {
    int32_t code, hori_offset, hori_count, vert_offset, vert_count;
} ftc_text_bank_entry;

/* The bank: 32 bytes.  rows and table are device addresses. */
typedef struct ftc_text_bank {
    const uint16_t* rows;             /* fp16 [n_rows][100] */
    const ftc_text_bank_entry* table; /* [n_codes] */
    int32_t n_rows, n_codes;
    uint32_t valid;
    int32_t reserved;
} ftc_text_bank;

/* One sample: 96 bytes, no padding.  The four pointers are device addresses or null (use the seed). */
typedef struct ftc_text_sample_desc {
    const int32_t* pick; /* [n_chars] */
    const double* n;     /* [400][100] */
    const double* z;     /* [400][100] */
    const double* u;     /* [400] */
    uint64_t seed_pick, seed_n, seed_z, seed_u;
    double noise_ratio, p;
    int64_t text_offset; /* the sample's first character in `chars` */
    int32_t n_chars;
    int32_t flags;
} ftc_text_sample_desc;

#ifdef __cplusplus
static_assert(sizeof(ftc_text_bank_entry) == 20, "ftc_text_bank_entry is a fixed 20-byte record");
static_assert(sizeof(ftc_text_bank) == 32, "ftc_text_bank is a fixed 32-byte record");
static_assert(sizeof(ftc_text_sample_desc) == 96, "ftc_text_sample_desc is a fixed 96-byte record");
#else
_Static_assert(sizeof(ftc_text_bank_entry) == 20, "ftc_text_bank_entry is a fixed 20-byte record");
_Static_assert(sizeof(ftc_text_bank) == 32, "ftc_text_bank is a fixed 32-byte record");
_Static_assert(sizeof(ftc_text_sample_desc) == 96, "ftc_text_sample_desc is a fixed 96-byte record");
#endif

int ftc_text_sample_abi_version(void);

/* Validates table_host (n_codes records) against n_rows and fills *bank; host work only.  Refused (bank->valid stays 0): a null bank, rows_dev,
   table_host or table_dev, n_codes < 1, n_rows < 1, a negative code, codes not strictly ascending, a negative offset or count,
   offset + count > n_rows. */
int ftc_text_bank_init(ftc_text_bank* bank, const uint16_t* rows_dev, const ftc_text_bank_entry* table_host, const ftc_text_bank_entry* table_dev,
                       int n_codes, int n_rows);

/* The batch.  descs_host / descs_dev hold the SAME B records; chars is the device array of all texts (int32 code points, total_chars of
   them), sample b reading chars[text_offset .. text_offset + n_chars - 1].  1 <= B <= 65536.  Refused (negative status, nothing enqueued,
   the outputs untouched): a null bank, descs_host, descs_dev, feature, in_codes or out_codes; a bank not marked valid; B outside its range;
   total_chars < 0; chars null with total_chars > 0; per record: n_chars < 0, n_chars > FTC_TEXT_SAMPLE_MAX_CHARS, text_offset < 0,
   text_offset + n_chars > total_chars, unknown flags, a noise_ratio or p that is NaN. */
int ftc_text_sample(const ftc_text_bank* bank, const ftc_text_sample_desc* descs_host, const ftc_text_sample_desc* descs_dev, int B,
                    const int32_t* chars, int64_t total_chars, void* feature, int feature_fp32, int64_t* in_codes, int64_t* out_codes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
