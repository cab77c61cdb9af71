// Prints the request launch's hint set (mirbft_amd/csrc/mirsha_hints.h, plain
// C++) for every length in [0, max_len] at the strides given, one line per
// (length, stride): tests/test_uniform_hint_host.py checks each field against
// FIPS 180-4 padding worked out independently in Python.
//   uniform_hint_unit <max_len> <stride> [<stride> ...]   (stride "L": the length itself)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mirsha_hints.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const unsigned max_len = (unsigned)strtoul(argv[1], nullptr, 10);
    for (int a = 2; a < argc; a++) {
        for (unsigned L = 0; L <= max_len; L++) {
            const unsigned long long stride = strcmp(argv[a], "L") == 0 ? L : strtoull(argv[a], nullptr, 10);
            const mirsha::UniformHint h = mirsha::make_uniform_hint(L, stride);
            printf("%u %llu %u %u %u %u %u %u %u %u %u", L, stride, h.valid, h.len, h.stride, h.nb, h.loop_nb, h.tail,
                   h.tail_bytes, h.tail_pad, h.reach);
            for (int k = 0; k < 4; k++) printf(" %u", h.keep[k]);
            for (int k = 0; k < 4; k++) printf(" %u", h.mark[k]);
            const mirsha::HintTail& t = h.tw;
            printf(" %u %u %u %u %u %u %u %u %u %u %u\n", t.kw4, t.kw14, t.kw15, t.c4, t.c14, t.c15, t.cs16, t.cs17,
                   t.cs19, t.cs29, t.cs30);
        }
    }
    return 0;
}
