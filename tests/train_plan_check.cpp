// Stand-alone driver of the pure functions of csrc/train_plan.h, built by the host compiler (tests/test_train_plan_cpu.py).
// Reads one request per line from standard input and answers each with one line:
//   P chunked chunk_barrier first first_wide resume_wide wide_from weighted limited multi vocab_size n_prior
//       -> rc route slot_vocab barrier <tab> message          (plan_begin; route 0 Slot, 1 SlotThenWide, 2 WideDirect)
//   B entries                 -> ok bits                       (table_bits)
//   H top positions merges    -> entries                       (wide_headroom)
// It decides nothing itself: the cases and what they must give are the test's.
#include "train_plan.h"

#include <cinttypes>
#include <cstdio>

using namespace mbpe;

int main() {
    char op;
    unsigned long long n_lines = 0;
    while (scanf(" %c", &op) == 1) {
        if (op == 'P') {
            long long v[11];
            for (long long &x : v)
                if (scanf("%lld", &x) != 1) return 2;
            const BeginIn in = {v[0] != 0, v[1], v[2], v[3], v[4], v[5], v[6] != 0, v[7] != 0, v[8] != 0, (uint32_t)v[9], (uint32_t)v[10]};
            const BeginPlan p = plan_begin(in);
            printf("%d %d %" PRIu32 " %d\t%s\n", p.rc, (int)p.route, p.slot_vocab, p.barrier ? 1 : 0, p.message.c_str());
        } else if (op == 'B') {
            unsigned long long e;
            if (scanf("%llu", &e) != 1) return 2;
            uint32_t bits = 0;
            const bool ok = table_bits(e, &bits);
            printf("%d %" PRIu32 "\n", ok ? 1 : 0, bits);
        } else if (op == 'H') {
            unsigned long long top, positions, merges;
            if (scanf("%llu %llu %llu", &top, &positions, &merges) != 3) return 2;
            printf("%" PRIu64 "\n", wide_headroom(top, positions, (uint32_t)merges));
        } else {
            return 2;
        }
        ++n_lines;
    }
    fprintf(stderr, "%llu requests\n", n_lines);
    return 0;
}
