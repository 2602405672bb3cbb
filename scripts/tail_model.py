"""Schedule model of the work-queue launch with level tickets (CPU only).

    python scripts/tail_model.py [--config C2] [--slots 1024] [--k 0,1024,2048,3072,4096,all] [--group 1,2,3]
                                 [--handover 50000:14000,20000:6000] [--out profiles/tail_groups_model.jsonl]

(profiles/tail_levels_model.jsonl of §3.12: --group 1 --handover 6000:1500,24000:6000.)  The hand-over defaults are
the measured ones: 50 k + 14 k cycles with the acquire-release fetch-adds under explicit fences that §3.12
shipped, and the 20 k + 6 k estimated for the fence pair of §3.13 (the guide's figures for one release and one
acquire; DESIGN.md §3.13 says what the counters gave).

Per-level costs come from the C oracle: the bench batch solved with sqp_iters = 1 .. L on HPIPM's profile; the
differences of the QP iteration counts are each solve's interior-point iterations per SQP-RTI iteration (level),
and a solve whose sqp_iter stops short of L has no later levels.  A level costs LIN_CYCLES + IPM_CYCLES x its
interior-point iterations (the stamped build's constants, profiles/r11a_stamps_C2.txt).

simulate() is the event simulation of the protocol of csrc/mpcg_tail.h on `slots` resident waves: tickets are
drawn in order by whichever wave is free first; a whole-solve ticket runs every level of its solve; a level
ticket whose predecessor has finished loads the carry block (load cycles) and runs the level; one whose
predecessor has not finished falls through at once, and the predecessor's wave goes on in place when it gets
there; a level that does not end its solve saves the block (save cycles).  One JSON line per case."""
import argparse
import heapq
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN_CYCLES, IPM_CYCLES = 54.4e3, 80e3


def grouped(levels, group):
    """the levels' costs summed by ticket group (csrc/mpcg_tail.h): level 0 alone, then `group` levels per
    ticket, the last group possibly short.  group 1: the levels themselves"""
    if group <= 1:
        return levels
    return [c[:1] + [sum(c[i:i + group]) for i in range(1, len(c), group)] for c in levels]


def simulate(levels, slots, K, load=0.0, save=0.0, group=1):
    """levels: per solve the list of its levels' costs (batch order).  Returns (makespan, busy fraction,
    hand-overs): busy = the levels' cycles / (slots x makespan), hand-overs = levels started from a carry block.
    group > 1: a level ticket stands for that many levels after level 0 (the protocol is the same, on groups)."""
    levels = grouped(levels, group)
    B = len(levels)
    K = min(max(K, 0), B)
    D = B - K
    L = max((len(c) for c in levels), default=0)
    tickets = [("whole", s, 0) for s in range(D)] + [("level", D + j, lv) for lv in range(L) for j in range(K)]
    # events in time order: (time, wave, what the wave has just saved or None); a wave with nothing pending
    # draws the next ticket
    ev = [(0.0, w, None) for w in range(min(slots, max(B, 1)))]
    heapq.heapify(ev)
    done = set()       # (solve, level): finished and saved, the finisher has been at the word
    fell = set()       # (solve, level): the ticket was drawn before the predecessor finished
    handovers, end, nt = 0, 0.0, 0

    def run(t, w, s, lv):
        c = levels[s]
        t += c[lv]
        if lv + 1 < len(c):
            heapq.heappush(ev, (t + save, w, (s, lv)))   # the solve goes on: save, then the word
        else:
            heapq.heappush(ev, (t, w, None))             # the solve ends here

    while ev:
        t, w, pending = heapq.heappop(ev)
        end = max(end, t)
        if pending is not None:
            s, lv = pending
            done.add((s, lv))
            if (s, lv + 1) in fell:
                run(t, w, s, lv + 1)                     # second at the word: on in place
            else:
                heapq.heappush(ev, (t, w, None))         # first: the next level's ticket loads the block
            continue
        if nt >= len(tickets):
            continue                                     # the wave leaves
        kind, s, lv = tickets[nt]
        nt += 1
        c = levels[s]
        if kind == "whole":
            heapq.heappush(ev, (t + sum(c), w, None))
        elif lv >= len(c):
            heapq.heappush(ev, (t, w, None))             # the solve has ended: the ticket falls through
        elif lv > 0 and (s, lv - 1) not in done:
            fell.add((s, lv))                            # first at the word: nothing to do
            heapq.heappush(ev, (t, w, None))
        else:
            if lv > 0:
                t += load
                handovers += 1
            run(t, w, s, lv)
    work = float(sum(sum(c) for c in levels))
    return end, (work / (slots * end) if end > 0 else 1.0), handovers


def level_costs(cfg, profile="hpipm", nthreads=0):
    """per solve of the bench batch of `cfg`: the cost in cycles of every level it runs, and the IPM counts"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import oracle_py
    from parity_full import DEFAULT_SCENES, inputs
    lay, b = inputs(cfg, DEFAULT_SCENES[cfg])
    L = lay.sqp_iters
    qp = np.zeros((L + 1, len(b.xinit)), np.int64)
    it = np.zeros(len(b.xinit), np.int64)
    for n in range(1, L + 1):
        r = oracle_py.Oracle(lay, qp_profile=profile, sqp_iters=n).solve_batch(b.params, b.warm, b.xinit, nthreads=nthreads)
        qp[n], it = r["qp_iter"], r["sqp_iter"]
    per = np.diff(qp, axis=0).T                       # [solve][level]
    levels = [[LIN_CYCLES + IPM_CYCLES * int(per[s][lv]) for lv in range(int(it[s]))] for s in range(len(it))]
    return levels, per, it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--k", default="0,1024,2048,3072,4096,all")
    ap.add_argument("--group", default="1,2,3", help="levels per ticket after level 0, comma separated")
    ap.add_argument("--handover", default="50000:14000,20000:6000", help="load:save cycles, comma separated")
    ap.add_argument("--shuffles", type=int, default=3, help="also each case on this many shuffled batch orders")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tail_groups_model.jsonl"))
    a = ap.parse_args()
    levels, per, it = level_costs(a.config)
    B = len(levels)
    ran = [per[s][:it[s]] for s in range(B)]
    allq = np.concatenate(ran)
    head = {"config": a.config, "solves": B, "slots": a.slots, "lin_cycles": LIN_CYCLES, "ipm_cycles": IPM_CYCLES,
            "mean_ipm_per_level": [round(float(np.mean([r[lv] for r in ran if len(r) > lv])), 3) for lv in range(per.shape[1])],
            "ipm_per_qp": {"mean": round(float(allq.mean()), 3), "p90": int(np.percentile(allq, 90)),
                           "p99": int(np.percentile(allq, 99)), "max": int(allq.max())},
            "rti_per_solve": round(float(it.mean()), 3), "ipm_per_solve": round(float(np.mean([r.sum() for r in ran])), 2)}
    base, busy0, _ = simulate(levels, a.slots, 0)
    ideal = sum(sum(c) for c in levels) / a.slots
    head.update(makespan_whole_solves=base, busy_whole_solves=round(busy0, 4), ideal_vs_whole=round(ideal / base - 1, 4))
    lines = [head]
    for ho in a.handover.split(","):
        load, save = (float(x) for x in ho.split(":"))
        for G in (int(g) for g in a.group.split(",")):
            for ks in a.k.split(","):
                K = B if ks == "all" else int(ks)
                end, busy, n = simulate(levels, a.slots, K, load, save, G)
                rec = {"config": a.config, "K": K, "group": G, "load": load, "save": save,
                       "makespan_vs_whole": round(end / base - 1, 4), "busy": round(busy, 4), "handovers": n}
                sh = []
                for seed in range(a.shuffles):
                    o = np.random.default_rng(seed).permutation(B)
                    lv = [levels[i] for i in o]
                    sh.append(round(simulate(lv, a.slots, K, load, save, G)[0] / simulate(lv, a.slots, 0)[0] - 1, 4))
                rec["shuffled_orders_vs_whole"] = sh
                lines.append(rec)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))


if __name__ == "__main__":
    main()
