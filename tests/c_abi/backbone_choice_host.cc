// Host-only client of csrc/backbone_choice.h (no HIP header, no GPU).  Reads one request per line from standard input:
//   <kind letter> <the 24 int fields of an ftc_op, in the header's order> [<operand mask>]
// with the letter s (STEM), d (DWCONV), e (SE), m (MBHEAD), f (FMBCONV) or u (UPCAT) -- it must agree with the kind field -- and, optionally, which
// of the eleven operands are given (bit i = the i-th ftc_ref of the struct; a resolver reads nothing else of an operand).  Prints the reason the op
// is refused (empty = accepted), a tab, the label, a tab, what selects the kernel instantiation, a tab, what sizes the launch.
// tests/test_abi_and_plan.py builds it with -fsanitize=address,undefined, feeds it the sweeps of tests/backbone_choice_sweep.py and compares the lines with
// tests/golden/backbone_choices.json.gz.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../findtextcenternet_amd/csrc/backbone_choice.h"

int main() {
    using namespace backbone;
    static const char* const se_family[] = {"fc1+fc2", "fc1+fc2_fold", "fold64", "gates64", "foldx3", "fc2_hpart"};
    static const char* const ms_family[] = {"general", "map24", "band48"};
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
        const char* letters = "sdemfu";
        const int kinds[] = {FTC_OP_STEM, FTC_OP_DWCONV, FTC_OP_SE, FTC_OP_MBHEAD, FTC_OP_FMBCONV, FTC_OP_UPCAT};
        const char* at = std::strchr(letters, line[0]);
        if (!at || line[0] == 0 || kinds[at - letters] != op.kind) return 3;
        char buf[160];
        const char* why = nullptr;
        switch (op.kind) {
        case FTC_OP_STEM: {
            StemChoice c;
            if ((why = stem_resolve(op, &c))) break;
            stem_format_label(op, c, buf, sizeof buf);
            std::printf("\t%s\tfamily=%d out=%s copy=%s nq=%d fast=%d\ttotal=%ld blocks=%d lds=%d\n", buf, c.family, dtname(c.out_dtype), dtname(c.copy_dtype), c.nq, (int)c.fast,
                        c.total, c.blocks, c.lds_bytes);
            break;
        }
        case FTC_OP_DWCONV: {
            DwconvChoice c;
            if ((why = dwconv_resolve(op, &c))) break;
            dwconv_format_label(op, c, buf, sizeof buf);
            std::printf("\t%s\tfamily=%s T=%s stride=%d\ttilesX=%d P=%d tpw=%d grid=%u,%u,%u\n", buf, c.family == DW_STRIP ? "strip" : "general", dtname(c.dtype), c.stride,
                        c.tilesX, c.P, c.tpw, c.grid[0], c.grid[1], c.grid[2]);
            break;
        }
        case FTC_OP_SE: {
            SeChoice c;
            if ((why = se_resolve(op, &c))) break;
            se_format_label(op, c, buf, sizeof buf);
            std::printf("\t%s\tfamily=%s T=%s fc1=%d\tnz=%d grid=%u,%u,%u lds=%d fc1_grid=%u,%u fc1_lds=%d\n", buf, se_family[c.family], c.dtype < 0 ? "-" : dtname(c.dtype),
                        (int)!c.hpart, c.nz, c.grid[0], c.grid[1], c.grid[2], c.lds_bytes, c.fc1_grid[0], c.fc1_grid[1], c.fc1_lds_bytes);
            break;
        }
        case FTC_OP_MBHEAD: {
            MbheadChoice c;
            if ((why = mbhead_resolve(op, &c))) break;
            mbhead_format_label(op, c, buf, sizeof buf);
            std::printf("\t%s\tfamily=%s slice=%d T=%s\thpart=%d rows=%d R=%d nb=%d ns=%d nblk=%d lds=%d\n", buf, ms_family[c.family], c.slice, c.x3 ? "f16x3" : dtname(c.dtype),
                        (int)c.hpart, c.rows, c.R, c.nb, c.ns, c.nblk, c.lds_bytes);
            break;
        }
        case FTC_OP_FMBCONV: {
            FmbconvChoice c;
            if ((why = fmbconv_resolve(op, &c))) break;
            fmbconv_format_label(op, c, buf, sizeof buf);
            std::printf("\t%s\tT=%s E=%d bk=%d sn=%d\tncb=%d nk=%d\n", buf, c.x3 ? "f16x3" : dtname(c.dtype), c.E, c.bk, c.x3 ? 0 : c.sn, c.ncb, c.nk);
            break;
        }
        default: {
            UpcatChoice c;
            if ((why = upcat_resolve(op, &c))) break;
            upcat_format_label(op, c, buf, sizeof buf);
            std::printf("\t%s\tT=%s TT=%s V=%d\ttotal=%ld nb=%u G=%d\n", buf, dtname(c.T), dtname(c.TT), c.V, c.total, c.nb, c.G);
        }
        }
        if (why) std::printf("%s\t\t\t\n", why);
    }
    return 0;
}
