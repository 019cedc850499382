"""GPU: amos_fmat_ransac_device and amos_pnp_ransac_device on the steered case table of tests/ransac_steering.py, where the returned model
is a chosen root of the 7-point cubic, a chosen P3P solution, a chosen slot of a 64-iteration round or an EPnP refit of a chosen inlier
count (tests/test_ransac_steering_cpu.py asserts from the census that every such cell is filled).  The model, the mask and the status are
held to the restatement bit for bit, as in test_gpu_fmat.py / test_gpu_pnp.py; every batch runs twice on its handle and gives the same
bytes.  One test per case family, a few launches of at most 64 problems each."""
import collections

import numpy as np
import pytest

import ransac_steering as rs
import test_gpu_fmat as gf
import test_gpu_pnp as gp

pytestmark = pytest.mark.gpu
MAXP = 1024


@pytest.fixture(scope="module")
def fm(gpu_lib):
    h = gpu_lib.FundamentalRansac(max_points=MAXP, max_problems=64)
    yield h
    h.close()


@pytest.fixture(scope="module")
def pnp(gpu_lib):
    h = gpu_lib.PnpRansac(max_points=MAXP, max_problems=64)
    yield h
    h.close()


def _check_family(fm, pnp, family):
    """Every problem of the family -- landed where it was steered or not -- in launches of <= 64 problems that share kind, max_iters and
    the presence of a select mask."""
    import torch
    groups = collections.defaultdict(list)
    for fam, cell, p, c, ok in rs.table_census():
        if fam == family:
            groups[(p["kind"], p["max_iters"], p["sel"] is not None)].append((cell, p, c))
    assert groups, family
    for (kind, max_iters, has_sel), rows in groups.items():
        for at in range(0, len(rows), 64):
            part = rows[at:at + 64]
            probs = [(p["p1"], p["p2"]) if kind == "fmat" else (p["obj"], p["img"]) for _, p, _ in part]
            sel = np.concatenate([p["sel"] for _, p, _ in part]) if has_sel else None
            run, same, handle = (gf._run_batch, gf._same, fm) if kind == "fmat" else (gp._run_batch, gp._same, pnp)
            got = run(torch, handle, probs, select=sel, max_iters=max_iters)
            again = run(torch, handle, probs, select=sel, max_iters=max_iters)
            for g, a, (cell, p, c) in zip(got, again, part):
                same(g, c["want"], (family, cell, p["target"]))
                assert g[2] == a[2] and g[0].tobytes() == a[0].tobytes() and g[1].tobytes() == a[1].tobytes(), (family, cell)
                if has_sel:
                    assert not g[1][p["sel"] == 0].any()


def test_fmat_every_root_at_slot_0(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "fmat_roots")


def test_fmat_geometries(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "fmat_geometries")


def test_fmat_slots_across_the_round_boundary(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "fmat_slots")


def test_fmat_redrawn_subset(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "fmat_redraw")


def test_fmat_ties(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "fmat_ties")


def test_select_mask(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "select")


def test_p3p_every_solution_index(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "p3p")
    _check_family(fm, pnp, "p3p_dead_slot0")


def test_pnp_slots_across_the_round_boundary(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "pnp_slots")


def test_epnp_refit_counts(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "refit")


def test_epnp_refit_fallback(gpu_lib, fm, pnp):
    _check_family(fm, pnp, "refit_fallback")
