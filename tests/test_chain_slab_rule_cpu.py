"""The slab rule of the chain forward dynamics (devplan.h, chain_slab_rows: read by the kernel for its pointers and by run_chain for the
allocation), checked on the host over the plans of every robot URDF (MIT Humanoid, Tello and JVRC-1 among them) by a stand-alone program built
with AddressSanitizer and UBSan (tests/cpp/chain_slab_check.cpp, `make slab-check`): regions inside the slab and apart from each other, no
input rows when the inputs live in registers, every other layout as it was."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "robot-models")
DRIVER = os.path.join(ROOT, "build", "slab_check", "chain_slab_check")


def test_slab_rule_over_real_plans():
    urdfs = [os.path.join(MODELS, n) for n in sorted(os.listdir(MODELS)) if n.endswith(".urdf")]
    wanted = [u for u in urdfs if any(k in os.path.basename(u) for k in ("mit_humanoid", "tello", "jvrc"))]
    assert len(wanted) >= 2, urdfs
    r = subprocess.run(["make", "-C", ROOT, "slab-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([DRIVER, *urdfs], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 findings" in r.stdout
    humanoid = [line for line in r.stdout.splitlines() if line.startswith("mit_humanoid.urdf fp32")]
    assert humanoid and "inputs in registers" in humanoid[0], r.stdout
