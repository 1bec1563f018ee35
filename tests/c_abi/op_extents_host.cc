// Host-only client of csrc/op_extents.h (no HIP header, no GPU).  Reads one request per line from standard input: the 24 int fields of an ftc_op, in the
// header's order, then which of the eleven operands are given (bit i = the i-th ftc_ref of the struct; op_extents reads nothing else of an operand).
// Prints the reason the op's form is refused (empty = accepted), a tab, and for each operand "<state>:<bytes>" (0 unused, 1 optional, 2 required).
// tests/test_op_extents_host.py builds it with -fsanitize=address,undefined, feeds it the ops of tests/op_extents_sweep.py and compares the lines with
// ftc_op_extents and with tests/golden/op_extents.json.gz.
#include <cstdio>
#include <cstring>

#include "../../findtextcenternet_amd/csrc/op_extents.h"

int main() {
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        int v[25], n = 0, used = 0;
        for (const char* q = line; n < 25 && std::sscanf(q, "%d%n", &v[n], &used) == 1; q += used) ++n;
        if (n != 25) return 2;
        ftc_op op = {};
        static_assert(sizeof(int) == 4 && offsetof(ftc_op, reserved0) == 23 * 4 && offsetof(ftc_op, in) == 24 * 4, "the int fields of ftc_op lead the struct");
        std::memcpy(&op, v, 24 * sizeof(int));
        ftc_ref* refs = &op.in;
        for (int i = 0; i < FTC_NUM_OPERANDS; ++i) refs[i].base = (v[24] >> i & 1) ? FTC_BASE_WORKSPACE : FTC_BASE_NULL;
        OpExtents e;
        const char* why = op_extents(op, &e);
        std::printf("%s\t", why ? why : "");
        for (int i = 0; i < FTC_NUM_OPERANDS; ++i) std::printf("%s%d:%lld", i ? " " : "", why ? 0 : (int)e.state[i], why ? 0LL : (long long)e.bytes[i]);
        std::printf("\n");
    }
    return 0;
}
