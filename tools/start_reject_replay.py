#!/usr/bin/env python3
"""What rejection at start (include/smc_hip.h: smc_set_start_reject) can save: CPU replay of a complete tempering run (the checker's
statements of Micmem_SMC_main.py:95-262) that, for a sample of the in-support proposals of every Metropolis sweep, evaluates the
look of MMOps::start_values as the device does - the threshold of smc_mm_reject_threshold against the sums of the solve groups of
EARLIER passes of the queue - and counts the items that would not be started and the solve work they stand for.

  passes:  the solve groups a chunk of the queue covers are started together (solve_sched.h: kExPerChunk = 2); with the golden
           data's groups (0+5), 1, 2, 3, 4 the passes are {0+5, 1}, {2, 3}, {4}.  Other placements of the looks are reported too.
  work:    190 x attempts + 1100 per solve (the cost of an attempt and of a start plus its dense outputs, in instructions), the
           shared replicate counted once.
  upper estimate: every sibling of an earlier pass counts as finished when the look happens, and the look itself is free.

Test infrastructure (uses oracle/ and the library's host function); not part of the product.  CPU only.

    python tools/start_reject_replay.py [N=20000] [sample=1000] > profiles/r08_start_reject_replay.log
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

ATTEMPT, SOLVE = 190.0, 1100.0


def main():
    O = g.load_oracle()
    L = g.load_package().lib()
    data = O.MMData.load()
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    n_sample = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    n_ex, n_t = data.n_ex, data.n_t
    groups = [(0, 5), (1,), (2,), (3,), (4,)]          # smc_mm_group_replicates on the golden data
    assert n_ex == 6 and data.S0[0] == data.S0[5] and np.array_equal(data.t[0], data.t[5])
    orders = {
        "current passes {0+5,1},{2,3},{4}": [[0, 1], [2, 3], [4]],
        "a look before every group, index order": [[0], [1], [2], [3], [4]],
        "a look before every group, descending S0": [[k] for k in np.argsort([-data.S0[gr[0]] for gr in groups])],
        "a look before every group, ascending S0": [[k] for k in np.argsort([data.S0[gr[0]] for gr in groups])],
        "one look after the replicate pair": [[0], [1, 2, 3, 4]],
    }
    t0 = time.time()
    out = O.run_smc(data, O.SMCSettings(n_particle=n), seed=11, record_mh=True, n_threads=os.cpu_count() or 1)
    print(f"CPU replay of one run, N = {n}, seed 11: {time.time() - t0:.0f} s, {out['step']} tempering steps, "
          f"{out['n_mutation_sweeps']} Metropolis sweeps; up to {n_sample} in-support proposals sampled per sweep")
    rs = np.random.RandomState(3)
    tot = {k: np.zeros(2) for k in orders}       # work saved, work
    n_sampled = n_bad = 0
    lk_after = None
    print("step sweep  gamma    in-support sampled  items not started  work saved   a cancelled proposal was accepted")
    sweep_no = 0
    for rec in out["records"]:
        gamma = rec.gamma_new
        lk_prev = out["sweeps"][0][1] if rec.step == 1 else lk_after
        anc = np.repeat(np.arange(n), rec.p_is)[:n]
        lk1 = np.empty(n)
        lk1[:len(anc)] = lk_prev[anc]
        for mh in rec.mh:
            sweep_no += 1
            prop, rr, lk2, p0, r = mh["proposals"], mh["rr"], mh["lk2"], mh["p0"], mh["r"]
            ins = np.nonzero(p0 == 1)[0]
            pick = ins if len(ins) <= n_sample else rs.choice(ins, n_sample, replace=False)
            sub = prop[pick]
            _, pred, _ = O.mm_loglik_batch(sub, data, want_pred=True)
            S = ((data.P_obs[None] - pred) ** 2).sum(axis=2)                       # (sample, n_ex)
            att = np.array([[O.rk45_solve(th[0], th[1], data.S0[gr[0]], data.t[gr[0]])[1]["n_attempts"] for gr in groups] for th in sub])
            T = np.array([L.smc_mm_reject_threshold(float(lk1[i]), float(gamma), float(rr[i]), float(prop[i, 2]), n_ex, n_t, 1.0, 1)
                          for i in pick])
            work = ATTEMPT * att + SOLVE                                           # (sample, groups)
            line = None
            for name, passes in orders.items():
                fin = np.zeros(len(pick))
                skipped = np.zeros(att.shape, dtype=bool)
                for ps in passes:
                    dead = fin >= T
                    for k in ps:
                        skipped[:, k] = dead
                    for k in ps:                                                   # what this pass publishes for the next look
                        for e in groups[k]:
                            fin = fin + np.where(dead, 0.0, S[:, e])
                bad = int((skipped.any(axis=1) & (r[pick] == 1)).sum())
                tot[name] += ((work * skipped).sum() * len(ins) / len(pick), work.sum() * len(ins) / len(pick))
                if line is None:                                                   # the current order: the per-sweep table
                    n_bad += bad
                    n_items = sum(len(groups[k]) for k in range(len(groups)))
                    not_started = sum(skipped[:, k].sum() * len(groups[k]) for k in range(len(groups)))
                    line = (f"{rec.step:4d} {sweep_no:5d}  {gamma:.4f}  {len(ins):10d} {len(pick):7d}  "
                            f"{100.0 * not_started / (n_items * len(pick)):15.1f} %  {100.0 * (work * skipped).sum() / work.sum():9.1f} %   "
                            f"{'YES: ' + str(bad) if bad else 'no'}")
                assert bad == 0, (name, rec.step, sweep_no)
            n_sampled += len(pick)
            print(line)
            lk1 = lk2 * r + lk1 * (1.0 - r)
        lk_after = lk1
    print(f"sampled proposals: {n_sampled}; cancelled proposals that were accepted ones: {n_bad} (asserted 0 for every placement)")
    print("solve work of all Metropolis sweeps (weighted by the in-support count) that is never started:")
    for name, (saved, work) in tot.items():
        print(f"  {name:45s} {100.0 * saved / work:5.1f} %")


if __name__ == "__main__":
    main()
