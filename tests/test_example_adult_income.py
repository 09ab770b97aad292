"""The reference's correctness anchor: deterministic-mode AUC reproducibility
on the adult-income-style workload (SURVEY §4 / BASELINE.md)."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_once():
    env = dict(os.environ)
    env.update(REPRODUCIBLE="1", EMBEDDING_STALENESS="1")
    # the golden constants below are the CPU engine's: keep the example on
    # the CPU when the machine has a GPU (its GPU twin is in test_gpu_e2e)
    env.update(HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    # ... and bitwise only for one thread count and one set of CPU code
    # paths: the CPU GEMMs split their reductions by thread count, and MKL /
    # oneDNN / ATen dispatch on the CPU's ISA.  Pin the thread count and the
    # portable code paths so every x86-64 machine computes the same bits.
    env.update(
        OMP_NUM_THREADS="8", MKL_NUM_THREADS="8",
        MKL_CBWR="COMPATIBLE", ATEN_CPU_CAPABILITY="default",
        DNNL_MAX_CPU_ISA="SSE41", ONEDNN_MAX_CPU_ISA="SSE41",
    )
    code = (
        "import sys; sys.path.insert(0, r'%s');"
        "sys.path.insert(0, r'%s');"
        "import train; a, b = train.main(epochs=1); print('AUCS', repr(a), repr(b))"
        % (os.path.join(REPO, "examples", "adult_income"), REPO)
    )
    out = subprocess.run(
        [sys.executable, "-c", code],
        cwd=os.path.join(REPO, "examples", "adult_income"),
        env=env, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("AUCS")][0]
    _, train_auc, test_auc = line.split()
    return train_auc, test_auc


# Pinned golden constants (the analog of the reference's
# CPU_TEST_AUC = 0.8928645493226243, examples/src/adult-income/train.py:23):
# a DETERMINISTICALLY-WRONG numerics regression now fails loudly instead of
# passing the run-to-run reproducibility check.  Captured 2026-10-20 on the
# synthetic stand-in dataset, world=1 CPU, REPRODUCIBLE=1, staleness=1, under
# the pinned environment above; identical bits on an Intel Xeon and on the
# host CPU of an MI355X machine.  (The 2026-09-14 constants,
# 0.8791403438530434 / 0.8963082277978777, held only for 8 threads on the
# AVX-512 machine they were captured on.)
CPU_TRAIN_AUC = "0.8791406334123999"
CPU_TEST_AUC = "0.8963062665929253"


@pytest.mark.timeout(1200)
def test_deterministic_auc_reproduces():
    a1 = _run_once()
    a2 = _run_once()
    assert a1 == a2, f"deterministic mode must reproduce bitwise: {a1} != {a2}"
    train_repr = a1[0].split("(")[-1].rstrip(")")
    test_repr = a1[1].split("(")[-1].rstrip(")")
    assert train_repr == CPU_TRAIN_AUC, (
        f"train AUC drifted from the golden constant: {train_repr} != "
        f"{CPU_TRAIN_AUC} — a cross-commit numerics regression"
    )
    assert test_repr == CPU_TEST_AUC, (
        f"test AUC drifted from the golden constant: {test_repr} != "
        f"{CPU_TEST_AUC}"
    )
