"""ORB_SLAM2::Fuse / FuseInNeighbors (amos-slam_amd/host/KeyFrameFuse.h) on a stand-in map against the host class: ORBmatcherFor::Fuse once per
target keyframe in the reference's order.  The final map must be identical in every field the harness returns: the point at every feature of
every keyframe; per point bad, replaced-by, the observations, Observations() and the descriptor; nFused per target."""
import numpy as np
import pytest

import host_fuse_binding as fb

pytestmark = pytest.mark.gpu


def run_both(m, targets, lst, th=3.0):
    before = fb.pool_handles()
    parent = fb.fuse_neighbors("parent", m, targets, lst, th)
    dropin = fb.fuse_neighbors("dropin", m, targets, lst, th)
    print(f"nFused parent {parent['n_fused']} drop-in {dropin['n_fused']}, host re-searches {dropin['n_host_searches']}")
    assert fb.same_state(dropin, parent) == []
    return dropin, parent, before


def test_fuse_in_neighbors_gives_the_sequential_loops_map(gpu_lib):
    m, targets, lst = fb.neighbors_map(21)
    n_list = 300
    assert [len(k["keys"]) for k in m.kfs[:5]] == [400] * 5 and sorted(set(lst))[0] == -1 and len(lst) > len(set(lst))
    dropin, parent, before = run_both(m, targets, lst)
    first = np.array([k["point_of"] for k in m.kfs[:5]])                  # the targets' features on entry
    final = dropin["kf_points"][:5, :400]
    is_list = lambda a: (a >= 0) & (a < n_list)
    assert ((first < 0) & is_list(final)).sum() >= 20                      # AddObservation
    gone = np.nonzero(dropin["bad"][:n_list] & (dropin["replaced_by"][:n_list] >= n_list))[0]
    assert len(gone) >= 5                                                  # Replace: a list point gives way to the keyframe's point
    won = np.nonzero(is_list(dropin["replaced_by"][n_list:]))[0]
    assert len(won) >= 5                                                   # Replace: the keyframe's point gives way to a list point
    bad_owner = m.points["bad"][np.maximum(first, 0)].astype(bool) & (first >= 0)
    assert bad_owner.sum() >= 5 and dropin["n_fused"].sum() > 100          # features held by a bad point were among the candidates
    changed = (dropin["desc"][:n_list] != m.points["desc"][:n_list]).any(1) & ~dropin["bad"][:n_list].astype(bool)
    assert changed.sum() >= 3 and dropin["n_host_searches"] >= 3           # survivors of a Replace, searched again in a later target
    # the stale records give another map: the re-search carries weight
    stale = fb.fuse_neighbors("stale", m, targets, lst)
    assert stale["n_host_searches"] == 0 and fb.same_state(stale, parent) != []
    # the drop-in's single form, once per target, is the same loop
    single = fb.fuse_neighbors("single", m, targets, lst)
    assert fb.same_state(single, parent) == []
    assert fb.pool_handles() - before <= 1                                 # one pooled handle serves the host class and the re-searches


def test_single_fuse_of_5000_points(gpu_lib):
    m, targets, lst = fb.single_map(33)
    assert len(lst) == 5000
    dropin, parent, _ = run_both(m, targets, lst)
    assert dropin["n_fused"][0] > 2000 and dropin["bad"].sum() > m.points["bad"].sum() + 100   # many Replace calls among the candidates


def test_scw_form(gpu_lib):
    m, targets, lst = fb.neighbors_map(45, n_targets=2, n_feat=300, n_list=200, decoys=0)
    T = m.kfs[0]["T"].astype(np.float64)
    scw = T.copy()
    scw[:3, :] *= 1.7                                                      # a Sim3 with a scale != 1
    own = m.kfs[0]["point_of"]
    own = own[(own >= 200)][:40]                                          # points the keyframe already holds: spAlreadyFound
    lst = [p for p in lst if p >= 0] + [int(p) for p in own]
    parent, dropin = fb.fuse_scw("parent", m, 0, scw, lst), fb.fuse_scw("dropin", m, 0, scw, lst)
    print(f"nFused parent {parent['n_fused']} drop-in {dropin['n_fused']}, replace points {(dropin['replace_point'] >= 0).sum()}")
    assert fb.same_state(dropin, parent) == []
    assert np.array_equal(dropin["replace_point"], parent["replace_point"])
    assert (dropin["replace_point"] >= 0).sum() >= 10 and dropin["n_fused"][0] > (dropin["replace_point"] >= 0).sum()
    assert (dropin["replace_point"][-len(own):] == -1).all()


def test_degenerate_cases(gpu_lib):
    m, targets, lst = fb.neighbors_map(57, n_targets=3, n_feat=120, n_list=60, decoys=0, mono=(1,), empty=(2,))
    assert len(m.kfs[2]["keys"]) == 0 and m.kfs[1]["u_right"] is None
    dropin, _, _ = run_both(m, targets, lst)                               # a target without features, a monocular one among stereo ones
    assert dropin["n_fused"][2] == 0 and dropin["n_fused"][1] > 0
    run_both(m, targets, [])                                               # an empty list
    run_both(m, [], lst)                                                   # no targets
    run_both(m, targets, [-1, -1])                                         # only NULL entries
