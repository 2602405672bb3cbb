// tail_groups.cpp -- the level-ticket protocol of csrc/mpcg_tail.h with grouped levels, driven from host threads
// (tests/test_tail_groups.py builds it plain and with -fsanitize=thread and runs it).
//
//   tail_groups [threads] [solves] [levels] [G] [K] [seed]
//
// A ticket stands for a group of SQP-RTI iterations ("levels"): group 0 is level 0, then groups of G levels, the
// last one possibly short (tail::groups, group_first, group_of).  Every thread is a "wave" and does what
// sqp_kernel's ticket loop and the solve body do: it draws tickets until tail::decode says END; a group ticket
// claims its boundary word, runs the group's levels up to the one for which tail::group_ends holds -- or to
// the solve's end, which may come in the middle of a group or in the short last one --, and a group that ends
// without ending the solve is followed by finish() on the word group_of(levels done - 1).  Checked: every level
// of every solve runs exactly once and in order, on the carry its predecessor left (a plain variable, so that
// ThreadSanitizer reports an access the boundary word does not order); the words end at 2 / 1 / 0 as the
// protocol says; the atomic operations, counted inside the atomic, are one per group ticket past group 0 plus
// one per finished group that goes on (a retry or a spin would show as more); every thread leaves on the
// ticket counter alone.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "mpcg_tail.h"

namespace {

namespace tail = mpcg::tail;

thread_local long g_atomic_ops = 0;
// (the host atomic keeps acquire-release read-modify-writes: ThreadSanitizer does not model stand-alone fences)
struct HostAtomic {
    static unsigned fetch_add(unsigned* p, unsigned v) {
        ++g_atomic_ops;
        return __atomic_fetch_add(p, v, __ATOMIC_ACQ_REL);
    }
};

uint64_t mix(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}

struct Solve {
    uint64_t carry = 0;   // plain: what a level hands to the next (the carry block, or the wave's own state)
    int levels_run = 0;   // plain: written by the level's runner only
    int end_level = 0;    // the level after which the solve ends
    bool finished = false;
};

uint64_t level_value(int s, int l, uint64_t c, int rounds) {
    uint64_t x = c ^ mix(((uint64_t)s << 20) | (uint64_t)l);
    for (int r = 0; r < rounds; ++r) x = mix(x + (uint64_t)r);
    return x;
}

// the mapping's own properties, for every G and level the words can hold
long check_mapping() {
    long bad = 0;
    for (int G = 1; G <= 4; ++G) {
        if (tail::groups(0, G) != 0 || tail::groups(1, G) != 1) ++bad;
        for (int L = 2; L <= 1 + (tail::MAX_LEVELS - 1) * G; ++L) {
            const int ng = tail::groups(L, G);
            if (tail::group_of(L - 1, G) != ng - 1) ++bad;  // the last level is in the last group
            int next = 0;
            for (int g = 0; g < ng; ++g) {
                const int f = tail::group_first(g, G);
                if (f != next || tail::group_of(f, G) != g) ++bad;
                const int size = g == 0 ? 1 : G;
                for (int l = f; l < f + size && l < L; ++l) {
                    if (tail::group_of(l, G) != g) ++bad;
                    if (tail::group_ends(l, G) != (l == f + size - 1)) ++bad;
                }
                next = f + size;
            }
            if (next < L) ++bad;
            if (G == 1 && ng != L) ++bad;  // one level per group: the numbering without groups
        }
    }
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 8;
    const int batch = argc > 2 ? atoi(argv[2]) : 300;
    const int L = argc > 3 ? atoi(argv[3]) : 10;
    const int G = argc > 4 ? atoi(argv[4]) : 2;
    int K = argc > 5 ? atoi(argv[5]) : batch;
    const uint64_t seed = argc > 6 ? strtoull(argv[6], nullptr, 10) : 1;
    if (threads < 1 || batch < 1 || L < 2 || G < 1 || K < 0) return 2;
    const int NG = tail::groups(L, G);
    if (NG > tail::MAX_LEVELS) return 2;
    if (K > batch) K = batch;
    const tail::Plan plan{batch, K, NG};
    const int D = batch - K;
    std::vector<Solve> solves((size_t)batch);
    for (int s = 0; s < batch; ++s) {
        const uint64_t h = mix(seed * 1000003ULL + (uint64_t)s);
        // one solve in five ends early: on its first level, at a group's end or in the middle of a group
        solves[(size_t)s].end_level = (h % 5 == 0) ? (int)((h >> 8) % (uint64_t)L) : L - 1;
    }
    std::vector<unsigned> words((size_t)(K > 0 ? K : 1) * tail::WORDS_PER_SOLVE, 0u);
    std::atomic<unsigned> queue{0};
    std::atomic<long> errors{0}, calls{0}, expected_calls{0}, tickets{0}, finished_groups{0};

    auto rounds = [&](int s, int l) { return 50 + (int)(mix(seed ^ mix(((uint64_t)s << 8) | (uint64_t)l)) % 400); };
    auto run_level = [&](int s, int l) -> bool {  // true: the solve goes on
        Solve& S = solves[(size_t)s];
        if (S.finished || S.levels_run != l) ++errors;  // once, in order
        S.carry = level_value(s, l, S.carry, rounds(s, l));  // random duration
        S.levels_run = l + 1;
        if (l == S.end_level) { S.finished = true; return false; }
        return true;
    };
    // the solve body called by levels: from level l0 to the end of l0's group or of the solve.  Returns the
    // count of levels done when the solve goes on (tail_more), else 0
    auto run_group = [&](int s, int l0) -> int {
        for (int l = l0; l < L; ++l) {
            if (!run_level(s, l)) return 0;
            if (tail::group_ends(l, G)) return l + 1 < L ? l + 1 : (++errors, 0);  // (end_level <= L - 1)
        }
        ++errors;  // (the last level ends the solve: not reached)
        return 0;
    };

    auto wave = [&]() {
        long my_expected = 0, my_tickets = 0, my_finished = 0;
        g_atomic_ops = 0;
        for (;;) {
            const unsigned t = queue.fetch_add(1u, std::memory_order_relaxed);
            const tail::Ticket tk = tail::decode(plan, t);
            if (tk.kind == tail::END) break;
            if (tk.kind == tail::WHOLE) {
                for (int l = 0; l < L; ++l)
                    if (!run_level(tk.sol, l)) break;
                continue;
            }
            const int j = tk.sol - D;
            if (tk.lvl > 0) { ++my_expected; ++my_tickets; }  // the claim of a group past the first is one operation
            if (!tail::claim<HostAtomic>(words.data(), j, tk.lvl)) continue;
            for (int l0 = tail::group_first(tk.lvl, G);;) {
                if (tail::group_of(l0, G) >= NG) { ++errors; break; }
                const int more = run_group(tk.sol, l0);
                if (more == 0) break;  // ended: the later words stay untouched
                ++my_expected;
                ++my_finished;         // one finish per group that goes on
                if (!tail::finish<HostAtomic>(words.data(), j, tail::group_of(more - 1, G))) break;
                l0 = more;             // second at the word: on in place
            }
        }
        calls += g_atomic_ops;
        expected_calls += my_expected;
        tickets += my_tickets;
        finished_groups += my_finished;
    };

    std::vector<std::thread> pool;
    for (int i = 0; i < threads; ++i) pool.emplace_back(wave);
    for (auto& th : pool) th.join();

    long bad = errors.load() + check_mapping();
    for (int s = 0; s < batch; ++s) {
        const Solve& S = solves[(size_t)s];
        if (!S.finished || S.levels_run != S.end_level + 1) { ++bad; continue; }
        uint64_t c = 0;
        for (int l = 0; l <= S.end_level; ++l) c = level_value(s, l, c, rounds(s, l));
        if (c != S.carry) ++bad;
    }
    // the word behind group g: 2 where both parties met (the solve went on past the group), 1 where only the
    // ticket of an ended solve's later group came by
    long want_finished = 0;
    for (int j = 0; j < K; ++j)
        for (int g = 0; g < NG - 1; ++g) {
            const unsigned w = words[tail::word_index(j, g)];
            const int e = solves[(size_t)(D + j)].end_level;
            const bool went_on = tail::group_first(g + 1, G) <= e;
            want_finished += went_on;
            if (w != (went_on ? 2u : 1u)) ++bad;
        }
    if (queue.load() < (unsigned)(D + NG * K + threads)) ++bad;  // every thread left on the counter alone
    // atomic operations = group tickets past group 0 + finished groups that go on, whatever the interleaving
    if (tickets.load() != (long)K * (NG - 1) || finished_groups.load() != want_finished) ++bad;
    if (calls.load() != expected_calls.load() || calls.load() != tickets.load() + finished_groups.load()) ++bad;
    std::printf("threads %d solves %d levels %d G %d (groups %d) K %d: atomic operations %ld = tickets %ld + finished "
                "groups %ld, errors %ld\n", threads, batch, L, G, NG, K, calls.load(), tickets.load(),
                finished_groups.load(), bad);
    return bad == 0 ? 0 : 1;
}
