// tail_protocol.cpp -- the level-ticket protocol of csrc/mpcg_tail.h driven from host threads
// (tests/test_tail_protocol.py builds it plain and with -fsanitize=thread and runs it).
//
//   tail_protocol [threads] [solves] [levels] [K] [seed]
//
// Every thread is a "wave": it draws tickets from one counter until tail::decode says END, exactly as
// sqp_kernel's ticket loop does (claim before the loads, finish after the saves, go on in place when second at
// the word).  A level's work is a few hundred rounds of arithmetic on the solve's carry value; some solves
// end early.  Checked: every (solve, level) runs exactly once and in order; the carry a level reads is the
// one its predecessor wrote (a plain, non-atomic variable: ThreadSanitizer reports any access the boundary
// word does not order); no call waits or retries (the atomic
// operations are counted inside the atomic itself: every thread issues exactly one per level ticket past level 0
// and one per level that goes on, however the threads interleave).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "mpcg_tail.h"

namespace {

// every atomic operation the protocol issues is counted here, per thread: a retry or a spin inside claim() or
// finish() would show as more operations than tickets and finished levels account for
thread_local long g_atomic_ops = 0;
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
    uint64_t carry = 0;   // plain: what a level hands to the next (the carry block)
    int levels_run = 0;   // plain: written by the level's runner only
    int end_level = 0;    // the level after which the solve ends (its loop's break)
    bool finished = false;
};

// level l of solve s on the carry c: the value the next level must see
uint64_t level_value(int s, int l, uint64_t c, int rounds) {
    uint64_t x = c ^ mix(((uint64_t)s << 20) | (uint64_t)l);
    for (int r = 0; r < rounds; ++r) x = mix(x + (uint64_t)r);
    return x;
}

}  // namespace

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 8;
    const int batch = argc > 2 ? atoi(argv[2]) : 300;
    const int L = argc > 3 ? atoi(argv[3]) : 10;
    int K = argc > 4 ? atoi(argv[4]) : batch;
    const uint64_t seed = argc > 5 ? strtoull(argv[5], nullptr, 10) : 1;
    if (threads < 1 || batch < 1 || L < 2 || L > mpcg::tail::MAX_LEVELS || K < 0) return 2;
    if (K > batch) K = batch;
    const mpcg::tail::Plan plan{batch, K, L};
    const int D = batch - K;
    std::vector<Solve> solves((size_t)batch);
    for (int s = 0; s < batch; ++s) {
        const uint64_t h = mix(seed * 1000003ULL + (uint64_t)s);
        // one solve in five ends early, some of them on their first level (a failed first QP)
        solves[(size_t)s].end_level = (h % 5 == 0) ? (int)((h >> 8) % (uint64_t)L) : L - 1;
    }
    std::vector<unsigned> words((size_t)(K > 0 ? K : 1) * mpcg::tail::WORDS_PER_SOLVE, 0u);
    std::atomic<unsigned> queue{0};
    std::atomic<long> errors{0}, calls{0}, expected_calls{0};

    auto run_level = [&](int s, int l) -> bool {  // true: the solve goes on
        Solve& S = solves[(size_t)s];
        if (S.finished || S.levels_run != l) ++errors;  // once, in order
        const uint64_t h = mix(seed ^ mix(((uint64_t)s << 8) | (uint64_t)l));
        S.carry = level_value(s, l, S.carry, 50 + (int)(h % 400));  // random duration
        S.levels_run = l + 1;
        if (l == S.end_level) { S.finished = true; return false; }
        return true;
    };

    auto wave = [&]() {
        long my_expected = 0;  // one operation per level ticket past level 0, one per level that goes on
        g_atomic_ops = 0;
        for (;;) {
            const unsigned t = queue.fetch_add(1u, std::memory_order_relaxed);
            const mpcg::tail::Ticket tk = mpcg::tail::decode(plan, t);
            if (tk.kind == mpcg::tail::END) break;
            if (tk.kind == mpcg::tail::WHOLE) {
                for (int l = 0; l < L; ++l)
                    if (!run_level(tk.sol, l)) break;
                continue;
            }
            const int j = tk.sol - D;
            if (tk.lvl > 0) ++my_expected;  // the claim of a level past the first is one operation, level 0's none
            if (!mpcg::tail::claim<HostAtomic>(words.data(), j, tk.lvl)) continue;
            for (int l = tk.lvl;; ++l) {
                if (!run_level(tk.sol, l)) break;              // ended: the later words stay untouched
                if (l + 1 >= L) { ++errors; break; }           // (end_level <= L - 1: not reached)
                ++my_expected;  // one finish per level that goes on
                if (!mpcg::tail::finish<HostAtomic>(words.data(), j, l)) break;
            }
        }
        calls += g_atomic_ops;
        expected_calls += my_expected;
    };

    std::vector<std::thread> pool;
    for (int i = 0; i < threads; ++i) pool.emplace_back(wave);
    for (auto& th : pool) th.join();

    // every solve ran its levels 0 .. end_level exactly once and in order, each on its predecessor's carry
    long bad = errors.load();
    for (int s = 0; s < batch; ++s) {
        const Solve& S = solves[(size_t)s];
        if (!S.finished || S.levels_run != S.end_level + 1) { ++bad; continue; }
        uint64_t c = 0;
        for (int l = 0; l <= S.end_level; ++l) {
            const uint64_t h = mix(seed ^ mix(((uint64_t)s << 8) | (uint64_t)l));
            c = level_value(s, l, c, 50 + (int)(h % 400));
        }
        if (c != S.carry) ++bad;
    }
    // the words: 2 where both parties met, 1 where the ticket of an ended solve's later level fell through,
    // never more
    for (int j = 0; j < K; ++j)
        for (int l = 0; l < L - 1; ++l) {
            const unsigned w = words[mpcg::tail::word_index(j, l)];
            const int e = solves[(size_t)(D + j)].end_level;
            if (w != (l < e ? 2u : 1u)) ++bad;
        }
    if (queue.load() < (unsigned)(D + L * K + threads)) ++bad;  // every thread left on the counter alone
    if (calls.load() != expected_calls.load()) ++bad;
    std::printf("threads %d solves %d levels %d K %d: atomic operations %ld, errors %ld\n", threads, batch, L, K,
                calls.load(), bad);
    return bad == 0 ? 0 : 1;
}
