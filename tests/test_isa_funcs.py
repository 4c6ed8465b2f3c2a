"""tools/isa_funcs.py, the per-function comparison behind tools/isa_diff.sh: a
function keeps its identity when functions before it are removed (its index in
the local labels, the loop comments and the label padding shifts), a changed
instruction is a difference, and --allow-missing excuses the named removal only."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_funcs.py")


def func(name, idx, mul="v_mul_f32_e32 v40, v3, v37"):
    label = f".LBB{idx}_2:"
    return "\n".join([
        "\t.text",
        f"\t.globl\t{name}                    ; -- Begin function {name}",
        f"{name}:                                ; @{name}",
        f"; %bb.0:",
        f"\ts_cbranch_execz .LBB{idx}_3",
        f"{label}{' ' * (40 - len(label))}; =>This Inner Loop Header: Depth=1",
        f"; %bb.1:{' ' * 30};   in Loop: Header=BB{idx}_2 Depth=1",
        f"\t{mul}",
        f"\ts_cbranch_scc1 .LBB{idx}_2",
        f".LBB{idx}_3:",
        "\ts_endpgm",
        f".Lfunc_end{idx}:",
        "                                        ; -- End function",
        f"\t.set {name}.num_vgpr, 41",
        "",
    ])


def run(tmp_path, new, old, *opts):
    (tmp_path / "new.s").write_text(new)
    (tmp_path / "old.s").write_text(old)
    r = subprocess.run([sys.executable, TOOL, *opts, str(tmp_path / "new.s"), str(tmp_path / "old.s")],
                       capture_output=True, text=True)
    return r.returncode, r.stdout


OLD = "".join(func(n, i) for i, n in enumerate(["k_a", "k_dead", "k_b"] + [f"k_{j}" for j in range(8)] + ["k_z"]))


def test_removed_function_shifts_indices_only(tmp_path):
    # k_dead goes: every later function's index falls by one, the index 10 becomes 9 (one digit less,
    # so the padding in front of its label's comment grows)
    names = ["k_a", "k_b"] + [f"k_{j}" for j in range(8)] + ["k_z"]
    new = "".join(func(n, i) for i, n in enumerate(names))
    rc, out = run(tmp_path, new, OLD)
    assert rc == 1 and "  missing: k_dead" in out and "differs" not in out
    assert "11 of 12 existing functions identical, 0 added" in out
    rc, out = run(tmp_path, new, OLD, "--allow-missing", "^k_dead$")
    assert rc == 0 and "  missing (allowed): k_dead" in out
    assert "11 of 12 existing functions identical, 1 missing as allowed, 0 added" in out


def test_allow_missing_excuses_only_its_pattern(tmp_path):
    names = ["k_a"] + [f"k_{j}" for j in range(8)] + ["k_z"]  # k_dead and k_b are gone
    new = "".join(func(n, i) for i, n in enumerate(names))
    rc, out = run(tmp_path, new, OLD, "--allow-missing", "^k_dead$")
    assert rc == 1 and "  missing: k_b" in out and "  missing (allowed): k_dead" in out


def test_changed_instruction_is_a_difference(tmp_path):
    names = ["k_a", "k_dead", "k_b"] + [f"k_{j}" for j in range(8)] + ["k_z"]
    new = "".join(func(n, i, "v_mul_f32_e32 v40, v37, v3" if n == "k_b" else "v_mul_f32_e32 v40, v3, v37")
                  for i, n in enumerate(names))
    rc, out = run(tmp_path, new, OLD, "--allow-missing", "^k_dead$")
    assert rc == 1 and out.count("differs") == 1 and "  differs: k_b" in out


def test_added_function_is_no_difference(tmp_path):
    new = OLD + func("k_new", 12)
    rc, out = run(tmp_path, new, OLD)
    assert rc == 0 and "12 of 12 existing functions identical, 1 added" in out and "  added: k_new" in out
