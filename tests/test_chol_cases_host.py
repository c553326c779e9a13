"""CPU checks of the exact-factor cases (tests/chol_cases.py) that tests/test_gpu_chol_exact.py runs
on the device:

  1. the case table against plan_steps / plan_s3 (lfm_host.cpp) under AddressSanitizer + UBSan
     (tests/native/chol_plan_check.cpp, a stand-alone program built here with the flags of
     tests/native/Makefile and run directly): every case's width list, per step the trailing tiles,
     the next width, bands or supertiles, and the helper's units; likewise the width list of each
     draw's schedule-1 factorisation. "This n reaches this regime" is a checked fact.
  2. the builder: Sigma = L0 L0^T exactly (asserted inside exact_factor in two summation orders),
     kappa as recorded, and numpy's own factor and log density within 0.01 of the bounds.
  3. the numpy restatement of the blocked algorithm, fault-free, within 0.01 of the bounds under
     the cases' width lists; and with one injected fault at a time, at least 10 bounds away in the
     log density and in the worst entry of L. Measured |d| / bound (log density; worst L entry):
       (a) depth-4 slice dropped        n 1409 w=1: 1.2e5; 1.7e7   n 1537 wide: 8.7e5; 1.6e7
                                        n 1791 wide: 2.4e4; 1.3e7
       (b) 64-row slab skipped          n 1409 w=1: 1.1e8; 7.5e7   n 1473 w=1: 2.8e6; 1.1e8
                                        n 1599 wide: 6.4e7; 7.6e7
       (c) tile updated twice           n 1408 w=1: 5.9e6; 1.2e8   n 2433 wide: 6.6e5; 6.6e7
       (e) next diagonal block short    n 1537 wide, after the w = 4, 5, 2 panels: 6.0e7, 2.8e7,
                                        1.5e5; 1.7e8, 1.7e8, 1.0e8   n 897 w=2: 7.5e7; 3.7e8
     These four kinds stay above 10 bounds everywhere they were tried; the smallest is 2.4e4.
  4. fault (d), Sigma rounded to fp32 on input, at every size of the table
     (test_fp32_input_at_every_size). The worst entry of L moves by 890 bounds or more and the
     worst element of a draw by 636 or more (both smallest at n = 2559, 1.6e4 and 2.0e4 at
     n = 129). The log density does NOT move reliably: the rounding errors enter it with random
     signs, and |d| / bound is 692 at n = 129, 75 at 1409, 13 at 1791, 21 at 2433, but 4.9 at 897,
     4.7 at 1152, 9.0 at 1536, 0.29 at 1537, 6.5 at 1665, 2.9 at 1792, 1.9 at 1793, 4.0 at 2304 and
     2.1 at 2559 (chol_cases.FP32_SCALAR_UNDER_10, with the rows concerned). At those sizes the
     scalar does not see an fp32 step on the input; the draws do, which is why every case of the
     table draws, the helper cases included. The scalar figure is therefore no margin for the
     bounds' constant: a tenth of the smallest ratio is below 1, so the constant may not rise at
     all, and it has not (c is as the bounds above state it). For the element-wise bound a tenth of
     the smallest ratio is 64.
  5. the defaults that chol_cases.knobs_of restates, against the sources' text.
"""

import os
import subprocess

import numpy as np
import pytest

from tests import chol_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. the plan table
def test_case_table_matches_the_plan_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "chol_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *san, "-pthread",
                        os.path.join(ROOT, "tests", "native", "chol_plan_check.cpp"),
                        os.path.join(ROOT, "dis_project_amd", "csrc", "lfm_host.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    draws = list(C.CASES)
    lines = [C.plan_input(c.name, c.n, c.env) for c in C.CASES]
    lines += [C.draw_plan_input("draw:" + c.name, c.n, c.env) for c in draws]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"chol_plan_check: all passed ({len(lines)} cases)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = {}
    for ln in r.stdout.splitlines():
        if " widths=" in ln:
            head, steps = ln.split(" steps=")
            name, n, Mp, nblk, widths = head.split()
            got[name] = (n, Mp, nblk, widths[len("widths="):], steps)
    assert len(got) == len(lines)
    for c in C.CASES:
        n, Mp, nblk, widths, steps = got[c.name]
        assert n == f"n={c.n}" and Mp == f"Mp={C.round_up(c.n + 1, 128)}"
        assert nblk == f"nblk={-(-c.n // 128)}"
        assert widths == c.widths, (c.name, widths)
        assert steps == c.steps, (c.name, steps)
    for c in draws:
        assert got["draw:" + c.name][3] == c.draw_widths, (c.name, got["draw:" + c.name][3])


def test_restated_defaults_match_the_sources():
    """chol_cases.knobs_of restates the library's defaults; they are read here from the text that
    sets them, so the table is not held against a stale copy when one of them changes."""
    import re

    def text(*path):
        with open(os.path.join(ROOT, *path)) as f:
            return f.read()

    csrc = ("dis_project_amd", "csrc")
    ctx = text(*csrc, "lfm_ctx.hip")
    for name, default in C.DEFAULTS.items():
        found = re.findall(r'env_int_api\("' + name + r'",\s*(-?\d+)\)', ctx)
        assert found and set(found) == {str(default)}, (name, found)
    assert 'k.w0 = std::max(1, env_int_api("LFM_W0", 1))' in ctx
    assert 'k.sched = env_int_api("LFM_SCHED", 3) == 1 ? 1 : 3' in ctx
    chol_h = text(*csrc, "lfm_chol.h")
    assert re.search(r"constexpr int WBULK = (\d+);", chol_h).group(1) == str(C.WBULK_S3)
    assert re.search(r"constexpr int SUPERTILE = (\d+);", chol_h).group(1) == "6"
    assert re.search(r"constexpr int NB = (\d+);", chol_h).group(1) == str(C.NB)
    sched = text(*csrc, "lfm_chol_sched.hip")
    assert f"const int wbulk = s3 ? (bordered ? WBORD : WBULK) : {C.WBULK_S1};" in sched
    assert (f"ctx->knobs.w2min >= 0 ? ctx->knobs.w2min : (s3 ? {C.W2MIN_S3} : {C.W2MIN_S1})"
            in sched)
    assert "pp.supertile = SUPERTILE;" in sched and "pp.side_cus = ctx->side_cus;" in sched
    # S3Params' own defaults (what chol_plan_check uses for a "-") are the environment's
    host_h = text(*csrc, "lfm_host.h")
    assert "int cus = 256, side_cus = 32;" in host_h and "int helper = 1;" in host_h
    assert "double helper_tc = 700, helper_min = 1200;" in host_h
    assert "tall_split = 2, supertile = 6;" in host_h
    assert C.CUS == 256


def test_case_table_reaches_what_the_issue_names():
    """Properties of the table itself, read off its literals."""
    by = C.CASE
    # every fall-through of plan_steps at the wide knobs, each at three sizes or more
    for nblk, widths in ((9, "1,4,4"), (11, "1,4,5,1"), (12, "1,4,5,2"), (13, "1,4,5,2,1"),
                         (14, "1,4,5,4"), (15, "1,4,5,5")):
        ns = {c.n for c in C.CASES if c.name.startswith(f"wide_b{nblk}_") and c.widths == widths}
        assert {128 * nblk - 127, 128 * nblk - 1, 128 * nblk} <= ns
    assert {by["wide_b13_n1599"].n, by["wide_b13_n1601"].n} == {128 * 12 + 63, 128 * 12 + 65}
    assert {c.n for c in C.CASES if not c.env} == {129, 1025, 1409, 1471, 1473, 1535, 1536, 1537}
    # w = 2 throughout; W0 = 2 starts two wide
    assert all(set(c.widths.split(",")[1:-1]) == {"2"} for c in C.CASES if c.name.startswith("w2_"))
    assert all(c.widths.startswith("2") for c in C.CASES if "LFM_W0" in c.env)
    # the helper cases have a helped step, and only they do
    for c in C.CASES:
        helped = [f for f in c.steps.split() if not f.endswith(":0")]
        assert bool(helped) == c.name.startswith("helper"), c.name
        assert all(f.split(":")[2] == "S" for f in helped)
    # wide panels meet a supertiled rest region and bands in one plan
    assert "S" in by["wide_b14_n1791"].steps and "B" in by["wide_b14_n1791"].steps
    # every case has a draw, and the device test's distinct draws reach every size of the table
    assert all(c.draw_widths for c in C.CASES)
    assert {c.n for c in C.draw_cases()} == {c.n for c in C.CASES}
    assert len({(c.n, c.draw_widths) for c in C.draw_cases()}) == len(C.draw_cases())
    assert set(C.FP32_SCALAR_UNDER_10) <= {c.n for c in C.CASES}
    assert {c.sched for c in C.CASES if "LFM_SCHED" in c.env} == {1}
    assert max(c.n for c in C.CASES) <= 2560


# ------------------------------------------------------------------ 2. the builder
@pytest.mark.parametrize("n, kappa", [(129, 4.2), (1409, 5.7), (1791, 6.3)])
def test_builder_is_exact_and_numpy_agrees(n, kappa):
    p = C.exact_factor(n)
    assert abs(p["kappa"] - kappa) <= 0.06
    assert not p["Sigma"].flags.writeable and C.exact_factor(n) is p
    l0 = p["L0"]
    assert np.max(np.abs(np.triu(l0, 1))) == 0 and np.max(np.abs(np.tril(l0, -1))) < 1 / 64
    assert np.all((np.diag(l0) >= 1) & (np.diag(l0) < 2))
    chol = np.linalg.cholesky(p["Sigma"])
    dl = float(np.max(np.abs(chol - l0))) / factor_bound(p)
    z = np.linalg.solve(chol, p["y"] - p["loc"])
    logp = -0.5 * (n * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(chol))) + z @ z)
    dv = abs(logp - p["truth"]) / C.logp_bound(p)
    print(f"n {n}: kappa {p['kappa']:.2f}, numpy factor {dl:.2e} bounds, log density {dv:.2e}")
    assert dl <= 0.01 and dv <= 0.01


def factor_bound(p):
    """Bound of one entry of the factor: c times its largest entry (the diagonal's, below 2)."""
    return p["c"] * float(np.max(np.diag(p["L0"])))


# ------------------------------------------------------------------ 3. the restatement
def run(n, widths, fault=None):
    p = C.exact_factor(n)
    L, z, logp = C.blocked_cholesky(p["Sigma"], p["y"] - p["loc"], widths, fault)
    return (float(np.max(np.abs(L - p["L0"]))) / factor_bound(p),
            abs(logp - p["truth"]) / C.logp_bound(p), float(np.max(np.abs(z - p["w"]))))


@pytest.mark.parametrize("name", ["default_n129", "default_n1409", "default_n1536",
                                  "wide_b13_n1537", "wide_b13_n1599", "wide_b14_n1791",
                                  "w2_b8_n897", "w0wide_b12_n1409", "helperwide_n2433"])
def test_restatement_without_a_fault_is_within_a_hundredth_of_the_bounds(name):
    c = C.CASE[name]
    dl, dv, dz = run(c.n, C.widths_of(c))
    print(f"{name}: factor {dl:.2e} bounds, log density {dv:.2e} bounds, max|z - w| {dz:.2e}")
    assert dl <= 0.01 and dv <= 0.01
    if c.draw_widths is not None and c.draw_widths != c.widths:
        dl, dv, _ = run(c.n, tuple(int(v) for v in c.draw_widths.split(",")))
        assert dl <= 0.01 and dv <= 0.01


def _faults():
    F = C.Fault
    out = []
    # (a) one depth-4 slice of one off-diagonal tile's update, at step 1 (w = 1, 4 and 4 deep)
    for name in ("default_n1409", "wide_b13_n1537", "wide_b14_n1791"):
        nblk = -(-C.CASE[name].n // 128)
        out.append(("a", name, F("slice", 1, nblk - 2, nblk - 3, 8)))
    # (b) the first slab of the last, ragged, block row skipped in step 0's update of a middle tile
    for name in ("default_n1409", "default_n1473", "wide_b13_n1599"):
        nblk = -(-C.CASE[name].n // 128)
        out.append(("b", name, F("slab", 0, 2 * (nblk - 1), nblk // 2)))
    # (c) a tile of the helper's tail (the last block row) updated twice at a helped step
    for name in ("helper_n1408", "helperwide_n2433"):
        nblk = -(-C.CASE[name].n // 128)
        out.append(("c", name, F("twice", 1, nblk - 1, nblk - 2)))
    # (d) Sigma rounded to fp32: test_fp32_input_at_every_size
    # (e) the next diagonal block updated without the panel's last block column: after the w = 4,
    # the w = 5 and the w = 2 panel of 1,4,5,2,1, and after a w = 2 panel of the w = 2 plan
    for step in (1, 2, 3):
        out.append(("e", "wide_b13_n1537", F("short", step)))
    out.append(("e", "w2_b8_n897", F("short", 1)))
    return out


@pytest.mark.parametrize("kind, name, fault", _faults(),
                         ids=[f"{k}-{n}-s{f.step}" for k, n, f in _faults()])
def test_injected_fault_moves_the_result_by_ten_bounds(kind, name, fault):
    c = C.CASE[name]
    dl, dv, dz = run(c.n, C.widths_of(c), fault)
    print(f"fault ({kind}) {name} {fault}: factor {dl:.3g} bounds, log density {dv:.3g} bounds, "
          f"max|z - w| {dz:.2e}")
    assert dl >= 10.0
    assert dv >= 10.0


def test_fp32_input_at_every_size():
    """Fault (d) at every size of the table, with numpy's Cholesky of the fp32-rounded Sigma (the
    fault is in the input, so the blocking does not matter). The worst entry of L and the worst
    element of a draw with unit normals move by at least 10 bounds (measured: 890 and 636 at the
    least, both at n = 2559) at every size. The log density moves by at least 10 bounds except at
    the sizes chol_cases.FP32_SCALAR_UNDER_10 records, where it must be what is recorded there:
    the draws are what sees an fp32 step."""
    under = {}
    for n in sorted({c.n for c in C.CASES}):
        p = C.exact_factor(n)
        L = np.linalg.cholesky(p["Sigma"].astype(np.float32).astype(np.float64))
        z = np.linalg.solve(L, p["y"] - p["loc"])
        logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
        logp = -0.5 * (n * np.log(2 * np.pi) + logdet + float(z @ z))
        dv = abs(logp - p["truth"]) / C.logp_bound(p)
        dl = float(np.max(np.abs(L - p["L0"]))) / factor_bound(p)
        one = np.ones((1, n))
        dd = float(np.max(np.abs((L - p["L0"]) @ one[0]) / C.draw_bound(p, one)[0]))
        print(f"fault (d) n {n}: log density {dv:.3g} bounds, factor {dl:.3g}, draw {dd:.3g}")
        assert dl >= 10.0 and dd >= 10.0, n
        if dv < 10.0:
            under[n] = dv
    assert set(under) == set(C.FP32_SCALAR_UNDER_10), under
    for n, dv in under.items():
        rec = C.FP32_SCALAR_UNDER_10[n]
        assert abs(dv - rec) <= 0.1 * rec + 0.05, (n, dv)
