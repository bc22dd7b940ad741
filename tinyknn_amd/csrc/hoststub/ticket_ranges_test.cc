// The handout arithmetic of tickets.h on the host (tests/test_ticket_ranges_cpu.py): for every N given on the
// command line one line "N lo0 lo1 ... lo8" with the bounds of the TK_TICKETS ranges, and for every start range one
// line "start s r0 r1 ... r7" with the order in which a wave that starts at range s walks the ranges.
#include <cstdio>
#include <cstdlib>

#include "../tickets.h"

static_assert(tk_range_lo(0, 0) == 0 && tk_range_lo(0, TK_TICKETS) == 0, "no blocks: empty ranges");
static_assert(tk_range_lo(1 << 30, TK_TICKETS) == 1 << 30, "the product is formed in 64 bits");
static_assert(tk_range_at(TK_TICKETS - 1, 1) == 0 && tk_range_at(13, 0) == 13 % TK_TICKETS, "cyclic, masked");

int main(int argc, char **argv)
{
    std::printf("tickets %d\n", TK_TICKETS);
    for (int a = 1; a < argc; a++) {
        const int N = std::atoi(argv[a]);
        std::printf("N %d", N);
        for (int r = 0; r <= TK_TICKETS; r++) std::printf(" %d", tk_range_lo(N, r));
        std::printf("\n");
    }
    for (int s = 0; s < TK_TICKETS; s++) {
        std::printf("start %d", s);
        // as ticketed_blocks walks: the start, then one step at a time
        int tk = tk_range_at(s, 0);
        for (int i = 0; i < TK_TICKETS; i++) {
            std::printf(" %d", tk);
            if (tk != tk_range_at(s, i)) return 2;      // stepping and indexing agree
            tk = tk_range_at(tk, 1);
        }
        std::printf("\n");
    }
    return 0;
}
