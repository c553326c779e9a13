"""The preconditions of tests/test_gpu_exact_mid.py, on the CPU and with numbers: every case of
the extended-precision fixtures (tests/golden/exact_grad.npz, exact_reduced.npz,
exact_posterior.npz, exact_posterior_c5cov.npz) fits the mid-size resident batch, none of them is
dropped, and the only ones that are not positive definite are mix at restarts 1 and 5. A fixture
regeneration that breaks one of these fails here, instead of leaving the GPU test with fewer
cases than it says it judges.

The rules are the planners' own: tests/native/mid_shapes_check.cpp runs plan_mid and
plan_mid_post (dis_project_amd/csrc/lfm_host.cpp) on the fixtures' shapes, built here as a
stand-alone program under AddressSanitizer + UBSan with the flags of tests/native/Makefile.
"""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import load_golden
from tests.test_gpu_exact_grad import ILL, mix_cases, una_cases
from tests.test_gpu_exact_posterior import B_RESTARTS, C_ROUNDS, c5_datas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# group: (n, G, m); m = 0 for the value-and-gradient groups (no posterior call). c's two entries
# are its latent and its gene predictor.
SHAPES = {"sub": (1024, 4, 0), "una": (129, 3, 0), "mix": (48, 4, 0), "c5": (28, 4, 0),
          "a": (28, 4, 20), "b": (129, 3, 45), "c_lat": (28, 4, 100), "c_gene": (28, 4, 80)}
# block columns of the augmented matrix, ceil((n + 1) / 64), and blocks of test rows
BLOCKS = {"sub": (17, 0), "una": (3, 0), "mix": (1, 0), "c5": (1, 0), "a": (1, 1), "b": (3, 1),
          "c_lat": (1, 2), "c_gene": (1, 2)}


@pytest.fixture(scope="module")
def gx():
    return load_golden("exact_grad")


@pytest.fixture(scope="module")
def px():
    g = load_golden("exact_posterior")
    g.update(load_golden("exact_posterior_c5cov"))
    return g


@pytest.fixture(scope="module")
def restarts():
    from dis_project_amd import configs

    return configs.c3_restarts(configs.c2(), 32)


def test_the_fixtures_have_the_shapes_the_gpu_test_registers(gx, px, restarts):
    """n, G and m of every group, from the data the GPU test registers and the models it packs."""
    from dis_project_amd import configs, dataset as ds
    from oracle import lfm_exact as E

    work = configs.grid_workload("exact", 4, 256, seed_params=2, seed_y=3)
    got = {"sub": (work.data.X.shape[0], E.submodel(restarts[0], 4)[0].num_genes, 0)}
    assert gx["sub_grad"].shape == (32, 3 * 4 + 2) and gx["sub_mll"].shape == (32,)
    una = una_cases(gx, restarts)
    assert [c[0] for c in una] == [0, 1, 2, 3] and gx["una_y"].shape == (4, 129)
    assert {(c[1].shape[0], c[2].shape[0], c[3].num_genes) for c in una} == {(129, 129, 3)}
    got["una"] = (129, 3, 0)
    mix = mix_cases(gx, restarts)
    assert {(c[1].shape[0], c[2].shape[0], c[3].num_genes) for c in mix} == {(48, 48, 4)}
    assert np.any(mix[0][1][:, 2] == 0) and np.any(mix[0][1][:, 2] != 0)  # latent and gene rows
    got["mix"] = (48, 4, 0)
    works = configs.c5_ablations()
    models = configs.c5_rounds([w.model for w in works], 16)
    assert len(works) == 15 and len(models) == 240 and gx["c5_grad"].shape == (240, 14)
    assert {(w.data.X.shape[0], w.data.X.shape[1]) for w in works} == {(28, 3)}
    assert {m.num_genes for m in models} == {4}
    got["c5"] = (28, 4, 0)
    assert px["a_x"].shape == (28, 3) and px["a_y"].shape == (28,) and px["a_v"].shape == (28,)
    assert px["a_mean"].shape == (32, 2, 20) and px["a_cov"].shape == (32, 2, 20 * 21 // 2)
    got["a"] = (28, 4, px["a_t"].shape[0])
    assert px["b_x"].shape == (129, 3) and px["b_y"].shape == (129,) and px["b_v"].shape == (129,)
    assert px["b_mean"].shape == (5, 2, 45) and px["b_cov"].shape == (5, 2, 45 * 46 // 2)
    assert tuple(int(r) for r in px["b_restarts"]) == B_RESTARTS
    got["b"] = (129, E.submodel(restarts[0], 3)[0].num_genes, px["b_t"].shape[0])
    datas = c5_datas()
    assert len(datas) == 15 and tuple(int(r) for r in px["c_rounds"]) == C_ROUNDS
    assert {np.asarray(ds.dataset_3d(d)[0]).reshape(-1, 3).shape[0] for d in datas} == {28}
    t_lat, t_gene = ds.generate_test_times(100), ds.generate_test_times_pred(20, 4)
    assert px["c_lat_mean"].shape == (45, t_lat.shape[0]) and px["c_lat_var"].shape == (45, 100)
    assert px["c_gene_mean"].shape == (45, t_gene.shape[0]) and px["c_unique"].shape == (80,)
    assert px["c_gene_cov"].shape == (45, 60 * 61 // 2)
    got["c_lat"], got["c_gene"] = (28, 4, t_lat.shape[0]), (28, 4, t_gene.shape[0])
    assert got == SHAPES


def test_nothing_is_dropped_and_only_mix_r1_r5_are_not_pd(gx, px):
    red = load_golden("exact_reduced")
    for key in ("sub_grad_dropped", "una_grad_dropped", "mix_grad_dropped", "c5_grad_dropped"):
        assert gx[key].size == 0, key
    assert red["sub_dropped"].size == 0 and red["c5_dropped"].size == 0
    for key in ("a_dropped", "a_not_pd", "b_dropped", "b_not_pd"):
        assert not np.any(px[key]), key
    assert px["a_dropped"].shape == (32, 2) and px["b_dropped"].shape == (5, 2)
    assert tuple(int(r) for r in gx["ill"]) == ILL == (1, 5, 10, 29)
    # mix: Sigma is not PD in exact arithmetic at restarts 1 and 5, PD at 10 and 29
    assert np.isfinite(gx["mix_mll"]).tolist() == [False, False, True, True]
    assert np.all(np.isnan(gx["mix_grad"][:2])) and np.all(np.isfinite(gx["mix_grad"][2:]))
    np.testing.assert_allclose(gx["mix_min_eig"][:2], [-0.15, -0.69], atol=0.01)
    assert np.all(gx["mix_min_eig"][2:] > 0)
    # every other value and gradient is there to be judged, and every bound is the issue's
    for pre in ("sub", "una", "c5"):
        assert np.all(np.isfinite(gx[pre + "_mll"])) and np.all(np.isfinite(gx[pre + "_grad"]))
    for pre, live in (("sub", slice(None)), ("una", slice(None)), ("mix", slice(2, 4)),
                      ("c5", slice(None))):
        assert np.all(gx[pre + "_mll_rtol"][live] == 1e-9), pre
        assert np.all(gx[pre + "_grad_rtol"][live] == 1e-8), pre
        assert np.all(gx[pre + "_scale"][live] > 0), pre
    for key in ("a_rtol", "b_rtol", "c_lat_rtol", "c_gene_rtol"):
        assert np.all(px[key] == 1e-9), key
    for key in ("a_mean", "a_cov", "b_mean", "b_cov", "c_lat_mean", "c_lat_var", "c_gene_mean",
                "c_gene_cov"):
        assert np.all(np.isfinite(px[key])), key


def test_sub_sits_exactly_at_the_cap():
    from dis_project_amd import farm, predict

    src = open(os.path.join(ROOT, "include", "lfm.h")).read()
    assert "#define LFM_MID_MAX_N 1024" in src and "#define LFM_MID_MAX_M 4096" in src
    assert farm.MidBatchEvaluator.MAX_N == SHAPES["sub"][0] == 1024
    assert predict.MidBatchPredictor.MAX_M == 4096
    # 17 block columns; the last starts at row 1024 = n: no column of Sigma in it (nlim == 0)
    nb = (1024 + 1 + 63) // 64
    assert nb == 17 and 1024 - (nb - 1) * 64 == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_plan_mid_and_plan_mid_post_take_every_group(tmp_path):
    """The planners on every group alone, on test_mixed_sizes_in_one_handle's batch and on
    test_posterior_mixed_sizes_one_handle's: accepted, with the block counts the GPU test states;
    one row more than sub is refused."""
    exe = str(tmp_path / "mid_shapes_check")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *san, "-pthread",
                        os.path.join(ROOT, "tests", "native", "mid_shapes_check.cpp"),
                        os.path.join(ROOT, "dis_project_amd", "csrc", "lfm_host.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")

    def plan(shapes):
        args = [str(v) for s in shapes for v in s]
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=env)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
        return r.returncode, r.stdout

    for group, shape in SHAPES.items():
        rc, out = plan([shape])
        assert rc == 0, (group, out)
        assert "limits MID_MAX_N 1024 MID_MAX_M 4096 MID_TILE 64" in out
        n, G, m = shape
        assert 1 <= n <= 1024 and n % G == 0 and (m == 0 or (1 <= m <= 4096 and m % G == 0))
        nb, mb = (int(v) for v in re.search(r"nb (\d+) mb (\d+)", out).groups())
        assert (nb, mb) == BLOCKS[group], (group, nb, mb)
    # the mixed handles of the GPU test
    rc, out = plan([SHAPES["sub"]] * 2 + [SHAPES["una"]] * 4 + [SHAPES["mix"]] * 4
                   + [SHAPES["c5"]] * 15)
    assert rc == 0, out
    assert [int(v) for v in re.findall(r"nb (\d+)", out)] == [17] * 2 + [3] * 4 + [1] * 19
    rc, out = plan([SHAPES["a"]] * 2 + [SHAPES["b"]] * 5)
    assert rc == 0, out
    assert re.findall(r"nb (\d+) mb (\d+)", out) == [("1", "1")] * 2 + [("3", "1")] * 5
    # and the planner does refuse what lies past the cap
    rc, out = plan([(1025, 1, 0)])
    assert rc == 1 and "1024" in out, out
