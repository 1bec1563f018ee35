// Host-only client of csrc/wgrad_choice.h (no HIP header, no GPU).  Reads one request per line from standard input:
//   o <the 24 int fields of an ftc_op, in the header's order>   ->  the reason the op is refused (empty = accepted), a tab, the label, a tab, the choice
//   s B Ho Wo Cout Cin ksize                                     ->  wgrad_splits
// The choice is printed as what selects a kernel instantiation (family, the template arguments the family has, the form of the gate, the
// reduction kernel) and, after a second tab, what sizes the launch.
// tests/test_abi_and_plan.py builds it with -fsanitize=address,undefined, feeds it the sweeps of tests/wgrad_choice_sweep.py and compares the
// lines with tests/golden/wgrad_choices.json.gz.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../findtextcenternet_amd/csrc/wgrad_choice.h"

int main() {
    using namespace wgradimpl;
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        int v[24], n = 0, used = 0;
        for (const char* q = line + 1; n < 24 && std::sscanf(q, "%d%n", &v[n], &used) == 1; q += used) ++n;
        if (line[0] == 's' && n == 6) {
            std::printf("%d\n", wgrad_splits(v[0], v[1], v[2], v[3], v[4], v[5]));
            continue;
        }
        if (line[0] != 'o' || n != 24) return 2;
        ftc_op op = {};
        static_assert(sizeof(int) == 4 && offsetof(ftc_op, reserved0) == 23 * 4, "the int fields of ftc_op lead the struct");
        std::memcpy(&op, v, sizeof v);
        WgradChoice c;
        const char* why = wgrad_resolve(op, &c);
        if (why) {
            std::printf("%s\t\t\n", why);
            continue;
        }
        char buf[160];
        wgrad_format_label(op, c, buf, sizeof buf);
        const bool generic = c.family == WGRAD_GENERIC, thin = c.family == WGRAD_THIN;
        std::printf("\t%s\tfamily=%d tile=%d w=%d x=%d dz=%d co=%d ks=%d bk=%d gate=%d wide=%d", buf, c.family, c.tile, thin ? -1 : c.w_dtype, generic || thin ? c.x_dtype : -1,
                    generic ? c.dz_dtype : -1, c.thin_co, c.thin_ks, c.bk, generic || c.family == WGRAD_RING ? c.gated + c.se_epi : 0, (int)c.reduce_wide);
        std::printf("\tchunk=%ld nseg=%d sps=%ld splits=%d grid=%u,%u,%u lds=%d KK=%d\n", c.chunk, c.nseg, c.steps_per_split, c.splits, c.grid[0], c.grid[1], c.grid[2],
                    c.lds_bytes, c.KK);
    }
    return 0;
}
