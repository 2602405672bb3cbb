// mpcg_tail.h -- level tickets for the last solves of a work-queue launch.
//
// The work queue of sqp_kernel hands out whole solves; when it runs dry every resident slot waits for the
// longest solve still running.  Here the last K solves of the batch are handed out one SQP-RTI iteration
// (a "level") per ticket, so the launch ends on the longest remaining chain of iterations instead.
//
// Ticket numbering, with D = batch - K and L levels per solve:
//   0 .. D-1          whole solves, as before
//   D + l K + j       level l of solve D + j  (level-major: every level 0 before any level 1)
//   >= D + L K        the wave leaves the loop
//
// Grouped levels: a ticket may stand for a group of consecutive SQP-RTI iterations instead of
// one -- group 0 is iteration 0 alone (its QP is the long one), then groups of G iterations, the last one
// possibly short (groups, group_first, group_of below).  Everything in this header then reads "group" for
// "level": Plan.L is the number of groups, Ticket.lvl the group, and a boundary word stands between two
// groups.  G = 1 is one iteration per ticket.
//
// Between level l and level l + 1 of a tail solve stands one boundary word, zero at launch.  Exactly two
// parties may add one to it: the wave that finished level l (after it saved the solve's carry block) and the
// wave that drew the ticket of level l + 1 (before it loads the block).  Whoever arrives second runs level
// l + 1: the finisher goes on in place with the state it holds, the ticket holder loads the block.  Whoever
// arrives first does nothing more for this solve.  A solve that has ended never touches its later words, so
// the holders of its later tickets arrive first and fall through.  Nobody waits: no call here loops or
// re-reads a word, and the loop over tickets ends on the ticket counter alone.
//
// The atomic operation is a template parameter, so that the same text runs on the device (agent-scope
// fetch-add, mpcg_sqp.h) and under host threads in tests/cpp/tail_protocol.cpp.
#pragma once

#if defined(__HIPCC__)
#define MPCG_TAIL_HD __host__ __device__
#else
#define MPCG_TAIL_HD
#endif

namespace mpcg {
namespace tail {

// levels a launch may split a solve into (boundary words per tail solve: MAX_LEVELS - 1, padded to 16)
constexpr int MAX_LEVELS = 16;
constexpr int WORDS_PER_SOLVE = 16;

struct Plan {
    int batch;  // solves of the launch
    int K;      // the last K of them by levels (0: none)
    int L;      // levels per solve (groups(pr.sqp_iters, G))
};

enum Kind { WHOLE = 0, LEVEL = 1, END = 2 };
struct Ticket {
    int kind;
    int sol;  // solve (WHOLE, LEVEL)
    int lvl;  // level (LEVEL)
};

// The groups of a solve of `iters` SQP-RTI iterations at G iterations per group after iteration 0, the first
// iteration of group g and the group that iteration `it` belongs to
MPCG_TAIL_HD constexpr int groups(int iters, int G) { return iters <= 1 ? iters : 1 + (iters - 2 + G) / G; }
MPCG_TAIL_HD constexpr int group_first(int g, int G) { return g <= 0 ? 0 : 1 + (g - 1) * G; }
MPCG_TAIL_HD constexpr int group_of(int it, int G) { return it <= 0 ? 0 : 1 + (it - 1) / G; }
// iteration `it` is the last of its group (of a group that is not cut short by the solve's end)
MPCG_TAIL_HD constexpr bool group_ends(int it, int G) { return it % G == 0; }

// K of a launch: none when the queue does not wrap (batch <= grid), when the solve has more levels than the
// words hold or fewer than two, else `want` clamped to the batch
MPCG_TAIL_HD inline int plan_k(int batch, int grid, int levels, int want) {
    if (batch <= grid || levels > MAX_LEVELS || levels < 2 || want <= 0) return 0;
    return want < batch ? want : batch;
}

MPCG_TAIL_HD inline Ticket decode(const Plan& p, unsigned t) {
    const unsigned D = (unsigned)(p.batch - p.K);
    if (t < D) return Ticket{WHOLE, (int)t, 0};
    // (L K <= MAX_LEVELS x batch: 32-bit arithmetic past the test)
    if (p.K <= 0 || (unsigned long long)t - D >= (unsigned long long)p.L * (unsigned)p.K) return Ticket{END, p.batch, 0};
    const unsigned r = t - D, l = r / (unsigned)p.K, j = r - l * (unsigned)p.K;
    return Ticket{LEVEL, (int)(D + j), (int)l};
}

// the word between level l and level l + 1 of tail solve j (0 <= l < L - 1)
MPCG_TAIL_HD inline unsigned word_index(int j, int l) { return (unsigned)j * WORDS_PER_SOLVE + (unsigned)l; }

// The holder of ticket (j, l): true when it is to run the level.  Level 0 is the holder's; for l > 0 it runs
// the level only if the finisher of level l - 1 has been here already (its carry block is then complete).
template <class Atomic>
MPCG_TAIL_HD inline bool claim(unsigned* words, int j, int l) {
    if (l == 0) return true;
    return Atomic::fetch_add(&words[word_index(j, l - 1)], 1u) == 1u;
}

// The wave that finished level l of tail solve j without ending the solve, after its carry block is saved:
// true when it is to run level l + 1 in place (the ticket of that level has been drawn and fell through).
template <class Atomic>
MPCG_TAIL_HD inline bool finish(unsigned* words, int j, int l) {
    return Atomic::fetch_add(&words[word_index(j, l)], 1u) == 1u;
}

}  // namespace tail
}  // namespace mpcg
