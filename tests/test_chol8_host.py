"""csrc/chol8.h, compiled for the host (tests/chol8_host_main.cpp: AddressSanitizer, UBSan, -ffp-contract=off, nothing
preloaded), against its numpy restatement tests/chol8_ref.py: the flag on every system, the solution bit for bit wherever the
flag is true (where it is false no caller reads the solution).  No GPU."""
import copy
import struct
import subprocess

import numpy as np
import pytest

import chol8_ref
import prep_fixtures as PF
import prep_ref
import refine_cases
import refine_ref
import uvfit_cases
import uvfit_ref
from host_program import build_host_program

LAM = 1e-3


def _refine_system():
    sc = refine_cases.scene("exact")
    tp, ev = refine_ref.template_planes(sc["tmpl"][:, 0], 4, 4), refine_ref.evidence_planes_f32(sc["logits"][:1], 4)
    S, _ = refine_ref.sums(sc["starts"][:1], tp, ev, refine_cases.H, refine_cases.W, 4, want_A=False)
    return refine_ref.lm_system(S[0], LAM)


def _uvfit_system():
    uv, _, _ = uvfit_cases.whole_inputs(uvfit_cases.whole_cases()[0])
    S, _, _ = uvfit_ref.sums(uv, None, None, uvfit_cases.H, uvfit_cases.W, uvfit_cases.WT, uvfit_cases.HT)
    A, g = uvfit_ref.assemble(S[0])
    for i in range(8):
        A[i][i] = A[i][i] + LAM * A[i][i]
    return A, g


def _prep_system():
    court = PF.court_poi("pitch")
    manual, _ = PF.exact_annotations(court, PF.fixture_thetas()[:1], seed=6, n_short=0, noise_px=2.0)
    use, dst = prep_ref.usable_points(manual[0]), manual[0] * 2 - 1
    h0, _ = prep_ref.dlt(court, dst, use)
    L, b, _ = prep_ref.gn_system(h0, court, dst, use, LAM)
    return L, b


def _good():
    """a well-conditioned system: M^T M + I of a fixed random M"""
    g = np.random.default_rng(8)
    M = g.normal(size=(12, 8))
    return (M.T @ M + np.eye(8)).tolist(), g.normal(size=8).tolist()


def _with(i, value):
    L, b = _good()
    L[i][i] = value
    return L, b


# (name, system, ok on entry, the flag the case is built to give)
def _cases():
    return [("diagonal", ([[float(i + 1) if i == k else 0.0 for k in range(8)] for i in range(8)], [float(3 - i) for i in range(8)]),
             True, True),
            ("refine-damped", _refine_system(), True, True),
            ("uvfit-damped", _uvfit_system(), True, True),
            ("prep-gauss-newton", _prep_system(), True, True),
            ("good", _good(), True, True),
            ("pivot0-zero", _with(0, 0.0), True, False),
            ("pivot3-negative", _with(3, -1.0), True, False),
            ("pivot7-nan", _with(7, float("nan")), True, False),
            ("inf-diagonal", _with(2, float("inf")), True, True),
            ("ok-false-on-entry", _good(), False, False)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "chol8")


def test_header_against_the_restatement(program):
    cases = _cases()
    lines = []
    for _, (L, b), ok_in, _ in cases:
        tokens = [float(L[i][k]).hex() for i in range(8) for k in range(i + 1)] + [float(v).hex() for v in b] + [str(int(ok_in))]
        lines.append(" ".join(tokens))
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    for (name, (L, b), ok_in, built_for), line in zip(cases, out):
        L, x = copy.deepcopy(L), list(b)
        ok = chol8_ref.chol8_solve(L, x, ok_in)
        got = line.split()
        print(f"chol8 {name}: ok {got[0]} (restatement {int(ok)})")
        assert ok is built_for, name
        assert got[0] == str(int(ok)), name
        if ok:
            assert got[1:] == [struct.pack(">d", v).hex() for v in x], name
