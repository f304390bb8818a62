"""Predicted time of one accepted attempt of the lone-chain block (csrc/mm_rk45.h: mm_fast_uniform_attempts) from the
per-instruction costs that tools/fp64_chain_probe.hip measured on one wave with one live lane
(profiles/lone_chain_probe.json), for the block in the tree and for its parent (tests/golden/fast_block_parent.txt).

What the probe says and this model uses: a lone wave pays the ISSUE cost of every instruction, dependent or not (a dependent
v_fma_f64 chain and eight interleaved ones both run at 4.4 cycles per instruction; v_rcp_f64 holds the issue for its whole
~16 cycles: three independent instructions behind it do not shorten the chain), so the order of the arithmetic is worth
nothing.  What is not flat is a conditional branch: in the probe's stream of independent v_fma_f64, ~20 cycles not taken,
~29 taken, and ~16 more where the instruction before it is the vector compare that writes its condition.  Those branch costs
are UPPER BOUNDS from a synthetic stream, not the block's: the model puts the parent's block at 0.359 us (measured: 0.3315,
profiles/ab_lone_chain.log; 0.325 in round 3) and the tree's at 0.296 (measured 0.3040), i.e. it prices the four branches
and four instructions that the tree saved at 152 cycles where 66 arrived.  The arithmetic part (everything but branches) is
the same ~640 cycles in both and carries over: tree measured 728 cycles = 640 + three branches and bookkeeping.

    python tools/lone_chain_model.py [probe.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fast_block_asm as F  # noqa: E402

MEASURED_US = {"parent": 0.3315, "tree": 0.3040}     # profiles/ab_lone_chain.log (round 3, r03_ab_fast_tail.log: 0.325)


def costs(probe):
    c = {k: v["cycles_per_instruction"] * v["instructions_per_group"] for k, v in probe["cases"].items()}   # cycles per group
    fma = c["ilp8"] / 8
    salu = (c["salu8"] - fma) / 8
    base = c["br_none"]
    out = {
        "fma": fma, "dep_fma": c["dep_fma"] / 8, "addmul": c["dep_add_mul"] / 8, "salu": salu,
        "rcp": c["rcp_shadow3"] - 4 * fma,                               # issue-blocking: the three fillers do not hide it
        "rcp_then_nop": c["rcp_use"] - fma,
        "trans_f32": (c["pow_f32"] - 3 * fma - 2 * salu) / 2,            # v_log_f32, v_exp_f32 (conversions and s_nop as above)
        "br_not_taken": c["scc_not_taken"] - base - salu,
        "br_taken": c["scc_taken"] - base - salu,
        "br_after_vcmp": c["br_adjacent"] - base - fma,                  # the branch directly behind its vector compare
        "br_far_vcmp": c["br_far"] - base - fma,
        "br_after_salu_mask": c["mask_or"] - base - 2 * fma - salu,
    }
    return out


def predict(block, k, verbose=False):
    """Cycles of the accepted path: no exit taken, not the first step after a rejection, budget left."""
    habs = F.vn("in", "habs")
    kind, trace = F.trace_path(block, lambda op, srcs: op in ("v_cmp_lt_f64", "s_cmp_eq_u32", "s_cmp_gt_i32")
                               and not (op == "v_cmp_lt_f64" and srcs[0][1] == habs))
    assert kind == "loop"
    total, parts, prev = 0.0, {}, None
    for ins, taken in trace:
        if taken is not None:
            if taken:
                c, what = k["br_taken"], "branch, taken"
            elif prev is not None and prev.op.startswith("v_cmp"):
                c, what = k["br_after_vcmp"], "branch behind its vector compare"
            elif prev is not None and prev.op in F.MASK_OPS:
                c, what = k["br_after_salu_mask"], "branch behind scalar mask arithmetic"
            else:
                c, what = k["br_not_taken"], "branch, not taken"
        elif ins.op == "v_rcp_f64":
            c, what = k["rcp"], "v_rcp_f64"
        elif ins.op in ("v_log_f32", "v_exp_f32"):
            c, what = k["trans_f32"], "v_log_f32 / v_exp_f32"
        elif ins.op.startswith("s_"):
            c, what = k["salu"], "scalar, s_nop"
        elif ins.op in ("v_add_f64", "v_mul_f64"):
            c, what = k["addmul"], "v_add_f64 / v_mul_f64"
        else:
            c, what = k["fma"], "other vector (v_fma_f64 rate)"
        n, s = parts.get(what, (0, 0.0))
        parts[what] = (n + 1, s + c)
        total += c
        prev = ins
    return total, parts, len(trace)


def main():
    root = F.ROOT
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "lone_chain_probe.json")
    with open(path) as f:
        probe = json.load(f)
    k = costs(probe)
    ghz = probe["lone_wave_clock_MHz"] / 1000.0
    print("lone wave clock %.3f GHz; cycles per instruction: " % ghz + ", ".join(f"{n} {v:.1f}" for n, v in k.items()))
    with open(os.path.join(root, "tests", "golden", "fast_block_parent.txt")) as f:
        parent = F.parse_block(f.read())
    res = {}
    for name, block in (("parent", parent), ("tree", F.parse_file())):
        total, parts, n = predict(block, k)
        res[name] = total
        print(f"{name}: {n} instructions on the accepted path, {total:.0f} cycles = {total / ghz / 1000:.4f} us per attempt")
        for what, (cnt, cyc) in sorted(parts.items(), key=lambda kv: -kv[1][1]):
            print(f"    {cnt:4d} x {what:38s} {cyc:7.1f} cycles")
    for name in ("parent", "tree"):
        us = res[name] / ghz / 1000
        print(f"{name}: predicted {us:.4f} us against {MEASURED_US[name]} us measured: {100 * (us / MEASURED_US[name] - 1):+.1f} %"
              + (f", {100 * (us / 0.325 - 1):+.1f} % against round 3's 0.325 (stop condition: within 10 %)" if name == "parent" else ""))
    print(f"saved: predicted {res['parent'] - res['tree']:.0f} cycles, measured "
          f"{(MEASURED_US['parent'] - MEASURED_US['tree']) * ghz * 1000:.0f}: the probe's branch costs are upper bounds, not the block's")
    print(f"dependent path alone = the whole block: a dependent chain costs {k['dep_fma']:.2f} cycles per v_fma_f64, "
          f"independent ones {k['fma']:.2f}; re-ordering the arithmetic is worth 0")
    print(f"tree against parent: {100 * (res['tree'] / res['parent'] - 1):+.1f} % (go/no-go: more than the 2.5 % build-to-build scatter)")


if __name__ == "__main__":
    main()
