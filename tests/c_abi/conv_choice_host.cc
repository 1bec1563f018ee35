// Host-only client of csrc/conv_choice.h (no HIP header, no GPU): conv_resolve + conv_format_label over every aux0 in 1..4095 on the five ops of
// part "every_aux0" of tests/conv_choice_sweep.py, in its order.  One line per entry: the reason the op is refused (empty = accepted), a tab, the label.
// tests/test_abi_and_plan.py builds it with -fsanitize=address,undefined and compares the lines with tests/golden/conv_choices.json.gz.
#include <cstdio>

#include "../../findtextcenternet_amd/csrc/conv_choice.h"

int main() {
    const int modes[5][4] = {{FTC_F32, FTC_F32, FTC_F32, 1}, {FTC_F32, FTC_F32, FTC_F32, 3}, {FTC_BF16, FTC_BF16, FTC_BF16, 1}, {FTC_BF16, FTC_BF16, FTC_F32, 3},
                             {FTC_BF16, FTC_F32, FTC_BF16, 1}};      // (w_dtype, in_dtype, out_dtype, ksize)
    for (const auto& m : modes) {
        ftc_op op = {};
        op.kind = FTC_OP_CONV; op.act = FTC_ACT_NONE; op.w_dtype = m[0]; op.in_dtype = m[1]; op.out_dtype = m[2]; op.res_dtype = FTC_F32;
        op.B = 2; op.H = op.W = op.Ho = op.Wo = 24; op.Cin = op.Cin_total = 256; op.Cout = op.Cout_total = 192; op.ksize = m[3]; op.stride = 1;
        for (int aux0 = 1; aux0 < 4096; ++aux0) {
            op.aux0 = aux0;
            convimpl::ConvChoice c;
            const char* why = convimpl::conv_resolve(op, &c);
            char buf[160];
            convimpl::conv_format_label(op, c, buf, sizeof buf);
            std::printf("%s\t%s\n", why ? why : "", buf);
        }
        op.aux0 = 0;
        if (conv_pinned_choice(op) <= 0 || conv_small_tile_choice() != 7) return 1;
    }
    return 0;
}
