"""The hand-written lone-chain block (csrc/mm_rk45.h: mm_fast_uniform_attempts) computes what its parent computed.

The block's asm text is value-numbered symbolically (tools/fast_block_asm.py): a register's value is the identity of
(opcode, modifiers and values of its operands), inputs are identified by the C expression bound to them, every compare is a
free boolean and every path of one trip of the loop is followed.  tests/golden/fast_block_parent.txt is the block of the
commit before the exit tests were re-scheduled, verbatim.  Re-naming and re-ordering are invisible here; a change of an
operand, an opcode, a modifier or the order of the roundings in a sum is not (test_planted_swap_is_caught)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fast_block_asm as F  # noqa: E402

COMMITTED = ("t", "y", "k0", "habs", "minstep", "attempts", "rejected", "budget")


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "fast_block_parent.txt")) as f:
        return F.parse_block(f.read())


@pytest.fixture(scope="module")
def tree():
    return F.parse_file()


def test_final_values_equal_the_parents_on_every_path(parent, tree):
    leaves = F.outcomes(tree)
    assert {k for _, k, _ in leaves} == {"exit", "loop"}
    for _, _, finals in leaves:
        assert set(COMMITTED) <= set(finals)
    assert F.differences(parent, tree) == []
    assert F.differences(tree, parent) == []


def test_early_exits_leave_the_loop_entry_state(tree):
    """Where the block ends with code 1 (the next attempt is mm_item_attempt's), nothing of that attempt is committed."""
    one, seen = F.vn("lit", "1"), 0
    for assign, kind, finals in F.outcomes(tree):
        if kind == "exit" and finals["code"] == one:
            seen += 1
            for name in COMMITTED:
                assert finals[name] == F.vn("in", name), f"`{name}` is committed before the exit under {assign}"
    assert seen >= 4    # step size below its minimum, output due, error norm < 2^-64, error norm >= 2^64


def test_no_use_directly_after_a_transcendental(tree):
    # F.outcomes raises BlockError where the instruction executed after a v_rcp_f64 / v_log_f32 / v_exp_f32 names its result
    F.outcomes(tree)
    n = sum(i.op in F.TRANSCENDENTAL for i in tree.insns())
    assert n == 9       # seven reciprocals (six stages and the error scale), one logarithm, one exponential
    text = open(os.path.join(ROOT, "tests", "golden", "fast_block_parent.txt")).read()
    bad = F.parse_block(text.replace('"v_mul_f64 %[num], %[nvm], %[acc]\\n"\n        "v_fma_f64 %[e], -%[den], %[r], 1.0\\n"',
                                     '"v_fma_f64 %[e], -%[den], %[r], 1.0\\n"\n        "v_mul_f64 %[num], %[nvm], %[acc]\\n"', 1))
    with pytest.raises(F.BlockError):
        F.outcomes(bad)


def test_every_written_register_is_declared(tree):
    named, fixed = F.written_registers(tree)
    outputs = {n for n, o in tree.operands.items() if o["out"]}
    assert named <= outputs, f"written but not an output: {sorted(named - outputs)}"
    assert "exec" not in fixed
    assert fixed <= set(tree.clobbers), f"written but not a clobber: {sorted(fixed - set(tree.clobbers))}"
    # an output that is only written must not share a register with an input: early clobber
    for n in named:
        assert tree.operands[n]["constraint"][0] == "+" or tree.operands[n]["constraint"].startswith("=&"), n


def test_planted_swap_is_caught(parent):
    """Two terms of stage 4's sum in the other order: the same multiset of instructions, another order of roundings."""
    with open(F.MM_RK45) as f:
        text = F.asm_statement(f.read(), "mm_fast_uniform_attempts")
    a, b = '"v_fma_f64 %[acc], %[k2], %[a53], %[acc]\\n"', '"v_fma_f64 %[acc], %[k3], %[a54], %[acc]\\n"'
    assert text.count(a) == 1 and text.count(b) == 1
    swapped = text.replace(a, "@").replace(b, a).replace("@", b)
    diff = F.differences(parent, F.parse_block(swapped))
    assert diff     # other value numbers for y, k0, h_abs - and for the compares of the error norm, hence other paths
    assert any("final value of `y`" in d for d in diff)
