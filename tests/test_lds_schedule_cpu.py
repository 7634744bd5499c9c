"""The LDS / slab schedules of the chain programs, checked on the host (tests/cpp/lds_schedule_check.cpp, `make lds-check`).

Latency mode runs the limbs below the floating base on different wavefronts of one workgroup; only SEG_BARRIER / RSEG_BARRIER
order them, and the plan compiler places LDS objects by live ranges in program order.  A GPU test of a timing race passes most
of the time whether or not the race exists, so this check is deterministic: the driver compiles every model with capi.cpp's
budgets and checks every finished chain program -- the eight latency-mode programs and the one-wavefront ones -- against an
access table derived from the kernels (races between wavefronts inside a barrier interval, def-use of every block in program
order, bounds).  Its self-test mutates copies of the programs and must flag each mutation.

Models: every robot URDF, every zoo() model, a generated family (chain_test_tree, 2 - 6 limbs, deep pairs on and off) and
TelloWithArms with the arms before the legs.  The family must contain the shape the round-6 review found racy -- one wavefront
owns two or more direct limbs, the last direct limb has kid chains and runs on another wavefront than an earlier limb -- for two
and four wavefronts, ABA and RNEA, read from the compiled programs, so that it keeps its teeth when the dealing heuristic moves."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "build", "lds_check", "lds_schedule_check")


def _blobs(tmp_path):
    from models import lds_family, tello_with_arms_arms_first, zoo

    paths = []
    for prefix, models in (("zoo_", zoo()), ("", {k: m.serialize() for k, m in lds_family().items()}),
                           ("", {"tello_with_arms_arms_first": tello_with_arms_arms_first().serialize()})):
        for name, blob in models.items():
            p = tmp_path / f"{prefix}{name}.grbd"
            p.write_bytes(blob)
            paths.append(str(p))
    return paths


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_chain_program_lds_schedules(tmp_path):
    r = subprocess.run(["make", "-C", ROOT, "lds-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    urdfs = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "robot-models", "*.urdf")))
    r = subprocess.run([DRIVER, "--self-test", *urdfs, *_blobs(tmp_path)], capture_output=True, text=True, timeout=600)
    out = r.stdout
    summary = [l for l in out.splitlines() if l.startswith(("programs checked", "self-test"))]
    print("\n".join(summary))
    findings = [l for l in out.splitlines() if re.search(r"findings [1-9]", l) or l.startswith("    ")]
    assert r.returncode == 0, "\n".join(findings[:60] + summary) + r.stderr[-2000:]

    m = re.search(r"programs checked (\d+), skipped (\d+), not built (\d+); findings (\d+)", out)
    assert m and int(m.group(4)) == 0
    assert int(m.group(1)) > 500, m.group(0)
    assert "self-test: 4 of 4 mutations flagged" in out, summary

    progs = re.findall(r"^(\S+) (\w+): checked, .*, shape (\d)", out, re.M)
    checked = {p for _, p, _ in progs}
    for p in ("chain32", "chain32w", "chain64", "rchain32", "rchain32w", "rchain64",
              "chain32p", "chain64p", "chain32q", "chain64q", "rchain32p", "rchain64p", "rchain32q", "rchain64q"):
        assert p in checked, f"no model has a {p} program"
    # the ADVICE shape, in the generated family and in TelloWithArms with the arms first
    shaped = {(model, p) for model, p, s in progs if s == "1"}
    for p in ("chain32p", "chain32q", "rchain32p", "rchain32q"):
        assert any(model.startswith("chain_tree_") and q == p for model, q in shaped), f"the family lost the shape in {p}"
    for p in ("chain32p", "rchain32p"):
        assert ("tello_with_arms_arms_first.grbd", p) in shaped
