// Host-only client of csrc/train_choice.h (no HIP header, no GPU).  Reads one request per line from standard input:
//   <kind letter> <the 24 int fields of an ftc_op, in the header's order> [<operand mask>]
// with the letter n (BNSTAT), a (BNACT), b (BNBWD), d (DWBWD) or e (SEBWD) -- it must agree with the kind field -- or l (any kind: the label alone) and,
// optionally, which of the eleven operands are given (bit i = the i-th ftc_ref of the struct; a resolver reads nothing else of an operand).  Prints the
// reason the op is refused (empty = accepted), a tab, the label, a tab, what selects the kernel instantiation, a tab, what sizes the launch.  Every Q is
// printed as train::with_quads hands it to a template: the value the launcher instantiates its kernel with.
// tests/test_abi_and_plan.py builds it with -fsanitize=address,undefined; tests/test_bn_operands_host.py, tests/test_se_operands_host.py and
// tests/test_exact_operands_host.py hold its answers to the launch arithmetic restated in Python.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../findtextcenternet_amd/csrc/train_choice.h"

template <int MAXQ = 64> static int as_template_argument(int Q) {
    return Q == 0 ? 0 : train::with_quads<MAXQ>(Q, [](auto q) { return (int)decltype(q)::value; });
}

int main() {
    using namespace train;
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        int v[25], n = 0, used = 0;
        for (const char* q = line + 1; n < 25 && std::sscanf(q, "%d%n", &v[n], &used) == 1; q += used) ++n;
        if (n != 24 && n != 25) return 2;
        ftc_op op = {};
        static_assert(sizeof(int) == 4 && offsetof(ftc_op, reserved0) == 23 * 4 && offsetof(ftc_op, in) == 24 * 4, "the int fields of ftc_op lead the struct");
        std::memcpy(&op, v, 24 * sizeof(int));
        ftc_ref* refs = &op.in;
        static_assert(offsetof(ftc_op, out2) == offsetof(ftc_op, in) + 10 * sizeof(ftc_ref), "the eleven operands follow each other");
        for (int i = 0; i < 11; ++i) refs[i].base = n == 25 && (v[24] >> i & 1) ? FTC_BASE_WORKSPACE : FTC_BASE_NULL;
        const char* letters = "nabde";
        const int kinds[] = {FTC_OP_BNSTAT, FTC_OP_BNACT, FTC_OP_BNBWD, FTC_OP_DWBWD, FTC_OP_SEBWD};
        char buf[160] = "";
        const bool labelled = format_label(op, buf, sizeof buf);
        if (line[0] == 'l') {
            std::printf("%s\t%s\t\t\n", labelled ? "" : "no label", buf);
            continue;
        }
        const char* at = std::strchr(letters, line[0]);
        if (!at || line[0] == 0 || kinds[at - letters] != op.kind || !labelled) return 3;
        const char* why = nullptr;
        switch (op.kind) {
        case FTC_OP_BNSTAT: {
            BnstatChoice c;
            if ((why = bnstat_resolve(op, &c))) break;
            std::printf("\t%s\tfamily=%s T=%s Q=%d\tM=%ld nchunk=%d grid=%u,%u final=%u\n", buf, c.family == BN_Q ? "q" : "scalar", dtname(c.dtype), as_template_argument(c.Q), c.M,
                        c.nchunk, c.grid[0], c.grid[1], c.final_grid);
            break;
        }
        case FTC_OP_BNACT: {
            BnactChoice c;
            if ((why = bnact_resolve(op, &c))) break;
            std::printf("\t%s\tfamily=%s TI=%s TO=%s TC=%s Q=%d\tP=%d res=%d grid=%u,%u,%u\n", buf, c.family == BN_Q ? "q" : "scalar", dtname(c.ti), dtname(c.to), dtname(c.tc),
                        as_template_argument(c.Q), c.P, (int)c.has_res, c.grid[0], c.grid[1], c.grid[2]);
            break;
        }
        case FTC_OP_BNBWD: {
            BnbwdChoice c;
            if ((why = bnbwd_resolve(op, &c))) break;
            std::printf("\t%s\tfast=%d TC=%s ZT=%s Q=%d\tM=%ld gs=%d nchunk=%d ach=%d accum=%d partial=%u,%u final=%u apply=%u,%u\n", buf, (int)c.fast, dtname(c.tc), dtname(c.zt),
                        as_template_argument(c.Q), c.M, c.gs, c.nchunk, c.ach, c.accum, c.partial_grid[0], c.partial_grid[1], c.final_grid, c.apply_grid[0], c.apply_grid[1]);
            break;
        }
        case FTC_OP_DWBWD: {
            DwbwdChoice c;
            if ((why = dwbwd_resolve(op, &c))) break;
            std::printf("\t%s\tdata=%s Q=%d weight=%s Q=%d\twant=%d grid=%u,%u nchunk=%d wgrid=%u,%u wfinal=%u\n", buf,
                        !c.data.present ? "-" : c.data.family == DW_Q ? "q" : "general", as_template_argument(c.data.Q), c.weight.present ? "q" : "-",
                        as_template_argument<16>(c.weight.Q), c.data.want, c.data.grid[0], c.data.grid[1], c.weight.nchunk, c.weight.grid[0], c.weight.grid[1], c.weight.final_grid);
            break;
        }
        default: {
            SebwdChoice c;
            if ((why = sebwd_resolve(op, &c))) break;
            std::printf("\t%s\tQ=%d\tpch=%d ds=%u,%u,%u prep=%u,%u hidden=%u,%u dmean=%u,%u w=%u,%u lds=%d bs=%lld dsp=%lld scratch=%lld\n", buf, as_template_argument(c.Q), c.pch,
                        c.ds_grid[0], c.ds_grid[1], c.ds_grid[2], c.prep_grid[0], c.prep_grid[1], c.hidden_grid[0], c.hidden_grid[1], c.dmean_grid[0], c.dmean_grid[1], c.w_grid[0],
                        c.w_grid[1], c.dmean_lds_bytes, (long long)c.bs_offset, (long long)c.dsp_offset, (long long)sebwd_scratch_floats(op.B, op.Cin, op.aux0));
        }
        }
        if (why) std::printf("%s\t%s\t\t\n", why, buf);
    }
    return 0;
}
