"""amos_match_reloc_pnp_batch_device on the GPU against the plain-Python restatement (tests/reloc_pnp_restatement.py), compared with == on
the bytes: every field of the result record, Tcw, the inlier row, d_match and d_found where there is a pose, and the generator state the
carried blob begins with -- over three iterate(5) calls per case, a reset, a batch over two frames, a disabled pair, the status bits, the
4097-correspondence refusal, and the chain SearchByBoW row -> PnP -> PoseOptimization -> SearchByProjection on resident arrays."""
import numpy as np
import pytest

import pnp_restatement as pr
import reloc_pnp_cases as rc
import reloc_pnp_restatement as rp

pytestmark = pytest.mark.gpu
f32 = np.float32
PAD = 0x5A  # what the outputs hold on entry


class Resident:
    """Frames and pairs uploaded once; every run() is one amos_match_reloc_pnp_batch_device call on the same carried state."""

    def __init__(self, pkg, frames, pairs, cap=rc.CAPACITY, matcher=None):
        """frames: list of kps arrays; pairs: list of dict(frame, bow_match [n of its frame], points)."""
        import torch
        self.torch, self.pkg, self.cap, self.pairs, self.frames = torch, pkg, cap, pairs, frames
        nf, npairs = len(frames), len(pairs)
        kps, counts = np.zeros((nf, cap), pkg.KP_DTYPE), np.zeros(nf, np.int32)
        for f, k in enumerate(frames):
            counts[f] = len(k)
            kps[f, :len(k)] = k
        self.off = np.concatenate([[0], np.cumsum([len(p["points"]) for p in pairs])]).astype(np.int32)
        total = max(int(self.off[-1]), 1)
        allp = np.zeros(total, pkg.RELOC_POINT_DTYPE)
        bow = np.full((npairs, cap), -1, np.int32)
        for k, p in enumerate(pairs):
            allp[self.off[k]:self.off[k + 1]] = p["points"]
            bow[k, :len(p["bow_match"])] = p["bow_match"]
        self.total = total
        self.d_kps, self.d_counts, self.d_points, self.d_bow = (self.up(a) for a in (kps, counts, allp, bow))
        self.state_bytes = pkg.reloc_pnp_state_bytes(cap)
        self.d_state = torch.full((npairs, self.state_bytes), 0xCD, dtype=torch.uint8, device="cuda")  # garbage: a reset must not read it
        self.mt = matcher or pkg.OrbMatcher()
        self.own = matcher is None

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def run(self, params):
        """-> (results [pairs], inlier [pairs][cap], match [pairs][cap], found [total], generator states [pairs])"""
        torch, pkg, npairs, cap = self.torch, self.pkg, len(self.pairs), self.cap
        self.d_result = torch.full((npairs, 104), PAD, dtype=torch.uint8, device="cuda")
        self.d_inlier = torch.full((npairs, cap), PAD, dtype=torch.uint8, device="cuda")
        self.d_match = torch.full((npairs, cap), -77, dtype=torch.int32, device="cuda")
        self.d_found = torch.full((self.total,), PAD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.mt.reloc_pnp_batch_device(self.d_kps.data_ptr(), self.d_counts.data_ptr(), len(self.frames), self.d_points.data_ptr(),
                                       [p["frame"] for p in self.pairs], self.off, self.d_bow.data_ptr(), rc.LEVEL_SIGMA2, params, cap,
                                       self.d_state.data_ptr(), self.d_result.data_ptr(), self.d_inlier.data_ptr(), self.d_match.data_ptr(),
                                       self.d_found.data_ptr())
        self.mt.sync()
        torch.cuda.synchronize()
        results = np.frombuffer(self.d_result.cpu().numpy().tobytes(), pkg.RELOC_PNP_RESULT_DTYPE)
        states = np.frombuffer(self.d_state.cpu().numpy()[:, :8].tobytes(), np.uint64)
        return results, self.d_inlier.cpu().numpy(), self.d_match.cpu().numpy(), self.d_found.cpu().numpy(), states

    def close(self):
        if self.own:
            self.mt.close()


def params_of(pkg, pair, seed, reset, **kw):
    return pkg.reloc_pnp_params([f32(x) for x in pair["K"]], seed, reset=reset, n_iterations=rc.N_ITERATIONS, **dict(rc.REFERENCE, **kw))


def assert_pair(got, k, res, pair, want, rng_state, what):
    """pair k of one device call against the restatement's Result: record, rows, paddings, match and found."""
    results, inlier, match, found, states = got
    n, cap = len(pair["kps"]), res.cap
    a, b = res.off[k], res.off[k + 1]
    print(what, {f: int(results[f][k]) for f in rc.RESULT_FIELDS})
    rc.assert_result_equal(results[k], inlier[k, :n], want, what)
    assert int(results["skipped"][k]) == 0
    assert not inlier[k, n:].any(), f"{what}: inlier padding"
    if want.has_pose:
        wm, wf = rp.match_and_found(want, pair["bow_match"], len(pair["points"]))
        assert np.array_equal(match[k, :n], wm) and (match[k, n:] == -1).all(), f"{what}: d_match"
        assert np.array_equal(found[a:b], wf), f"{what}: d_found"
    else:
        assert (match[k] == -77).all() and (found[a:b] == PAD).all(), f"{what}: d_match / d_found written without a pose"
    if rng_state is not None:
        assert int(states[k]) == rng_state, f"{what}: generator state"


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_three_calls_on_carried_state_equal_the_restatement(gpu_lib, name):
    pair, seed, want = rc.case(name)
    res = Resident(gpu_lib, [pair["kps"]], [dict(pair, frame=0)])
    for call, (w, rng) in enumerate(want):
        got = res.run([params_of(gpu_lib, pair, seed, reset=1 if call == 0 else 0)])
        assert_pair(got, 0, res, pair, w, rng, f"{name} call {call}")
    # reset = 1 reproduces the first call
    got = res.run([params_of(gpu_lib, pair, seed, reset=1)])
    assert_pair(got, 0, res, pair, want[0][0], want[0][1], f"{name} after reset")
    res.close()


def test_batch_of_eight_pairs_over_two_frames_equals_the_single_calls(gpu_lib):
    """Pairs 0 .. 7 alternate between two frames; every pair has its own points, row, seed and state.  Both frames hold the features of
    their pairs' scenes: a pair's row names only its own features."""
    names = ["n20", "n63", "clean40", "n15", "out70", "n200", "coplanar", "n9"]
    cases = [rc.case(nm) for nm in names]
    frames = [[], []]
    pairs = []
    for k, (pair, seed, want) in enumerate(cases):
        f = k % 2
        base = sum(len(x) for x in frames[f])
        frames[f].append(pair["kps"])
        pairs.append(dict(frame=f, base=base, points=pair["points"], bow=pair["bow_match"], K=pair["K"]))
    kps = [np.concatenate(x) for x in frames]
    assert max(len(k) for k in kps) <= 512
    for p in pairs:
        row = np.full(len(kps[p["frame"]]), -1, np.int32)
        row[p["base"]:p["base"] + len(p["bow"])] = p["bow"]
        p["bow_match"], p["kps"] = row, kps[p["frame"]]
    res = Resident(gpu_lib, kps, pairs, cap=512)
    wants = []
    for k, (p, (pair, seed, _)) in enumerate(zip(pairs, cases)):
        wants.append(rc.run_restatement(dict(kps=p["kps"], bow_match=p["bow_match"], points=p["points"], K=p["K"]), seed, n_calls=2))
    for rep in range(2):
        for call in range(2):
            got = res.run([params_of(gpu_lib, p, c[1], reset=1 if call == 0 else 0) for p, c in zip(pairs, cases)])
            for k, p in enumerate(pairs):
                w, rng = wants[k][call]
                assert_pair(got, k, res, p, w, rng, f"rep {rep} call {call} pair {k} ({names[k]})")
    # the same as the eight single calls: a pair in a batch equals the pair alone (its restatement is the same object either way), and
    # the pair alone on the device:
    for k in (0, 5):
        p = pairs[k]
        single = Resident(gpu_lib, [p["kps"]], [dict(p, frame=0)], cap=512, matcher=res.mt)
        got = single.run([params_of(gpu_lib, p, cases[k][1], reset=1)])
        assert_pair(got, 0, single, p, wants[k][0][0], wants[k][0][1], f"single pair {k}")
    res.close()


def test_disabled_pair_leaves_the_outputs_untouched(gpu_lib):
    pair, seed, want = rc.case("n20")
    res = Resident(gpu_lib, [pair["kps"]], [dict(pair, frame=0), dict(pair, frame=0)])
    before = res.d_state.cpu().numpy().copy()
    got = res.run([params_of(gpu_lib, pair, seed, reset=1, enabled=0), params_of(gpu_lib, pair, seed, reset=1)])
    results, inlier, match, found, _ = got
    assert int(results["skipped"][0]) == 1 and not np.frombuffer(results[0].tobytes(), np.uint8)[:96].any()
    assert (inlier[0] == PAD).all() and (match[0] == -77).all() and (found[res.off[0]:res.off[1]] == PAD).all()
    assert np.array_equal(res.d_state.cpu().numpy()[0], before[0])
    assert_pair(got, 1, res, pair, want[0][0], want[0][1], "the enabled pair beside it")
    res.close()


def test_status_bits_for_octave_and_match_index(gpu_lib):
    pair, seed, _ = rc.case("n20")
    pair = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pair.items()}
    feats = np.nonzero(pair["bow_match"] >= 0)[0]
    pair["kps"]["octave"][feats[0]] = len(rc.LEVEL_SIGMA2)
    pair["kps"]["octave"][feats[1]] = -1
    pair["bow_match"][feats[2]] = len(pair["points"])
    want = rc.run_restatement(pair, seed, n_calls=2)
    assert want[0][0].status == 3
    res = Resident(gpu_lib, [pair["kps"]], [dict(pair, frame=0)])
    for call, (w, rng) in enumerate(want):
        assert_pair(res.run([params_of(gpu_lib, pair, seed, reset=1 - call)]), 0, res, pair, w, rng, f"status call {call}")
    res.close()


def test_carried_state_of_other_inputs_starts_over(gpu_lib):
    """reset = 0 on a blob that is no state (garbage) or the state of a solver with another correspondence count: status bit 2 and the
    first call's result."""
    pair, seed, want = rc.case("n20")
    res = Resident(gpu_lib, [pair["kps"]], [dict(pair, frame=0)])
    results, inlier, _, _, states = res.run([params_of(gpu_lib, pair, seed, reset=0)])
    assert int(results["status"][0]) == 4 and int(states[0]) == want[0][1]
    assert results["Tcw"][0].tobytes() == want[0][0].Tcw.tobytes() and int(results["iterations"][0]) == want[0][0].iterations
    assert inlier[0, :len(pair["kps"])].tobytes() == want[0][0].inlier.tobytes()
    res.close()


def test_4097_correspondences_give_code_minus_3(gpu_lib):
    n = rp.MAX_CORRESPONDENCES + 1
    obj, img, _, _ = pr.scene(np.random.default_rng(3), n)
    kps = np.zeros(n, rc.KP)
    kps["x"], kps["y"] = img[:, 0], img[:, 1]
    points = np.zeros(n, rc.POINT)
    points["pos"] = obj
    pair = dict(kps=kps, bow_match=np.arange(n, dtype=np.int32), points=points, K=pr.K_TUM, frame=0)
    res = Resident(gpu_lib, [kps], [pair], cap=n + 3)
    results, inlier, match, found, _ = res.run([params_of(gpu_lib, pair, 1, reset=1)])
    assert int(results["code"][0]) == -3 and int(results["n_correspondences"][0]) == n and int(results["has_pose"][0]) == 0
    assert (inlier == PAD).all() and (match == -77).all() and (found == PAD).all()  # nothing else is written
    # one fewer is solved: 4096 correspondences, the limit itself
    pair["bow_match"] = pair["bow_match"].copy()
    pair["bow_match"][n - 1] = -1
    want = rc.run_restatement(pair, 1, n_calls=1)
    res2 = Resident(gpu_lib, [kps], [pair], cap=n + 3, matcher=res.mt)
    assert_pair(res2.run([params_of(gpu_lib, pair, 1, reset=1)]), 0, res2, pair, want[0][0], want[0][1], "4096 correspondences")
    res.close()


def test_host_form_equals_the_restatement(gpu_lib):
    """amos_match_reloc_pnp: one pair from host arrays, the state blob carried by the caller."""
    mt = gpu_lib.OrbMatcher()
    for name in ("n20", "n15", "n0", "out70"):
        pair, seed, want = rc.case(name)
        state = None
        for call, (w, rng) in enumerate(want):
            r, inlier, match, found, state = mt.reloc_pnp(pair["kps"], pair["bow_match"], pair["points"], rc.LEVEL_SIGMA2,
                                                          params_of(gpu_lib, pair, seed, reset=1 if call == 0 else 0), state)
            rc.assert_result_equal(r, inlier, w, f"host form {name} call {call}")
            assert int(np.frombuffer(state[:8].tobytes(), np.uint64)[0]) == rng
            if w.has_pose:
                wm, wf = rp.match_and_found(w, pair["bow_match"], len(pair["points"]))
                assert np.array_equal(match, wm) and np.array_equal(found, wf)
            else:
                assert match is None and found is None
    mt.close()


def test_chain_bow_pnp_pose_search(gpu_lib):
    """One lost frame, two candidate keyframes, resident arrays: amos_match_bow_batch_device -> amos_match_reloc_pnp_batch_device (its
    row is SearchByBoW's d_match as written) -> the host reads d_result and fills the pose cameras from Tcw ->
    amos_match_pose_optimization_batch_device on the PnP's d_match as written -> amos_match_reloc_batch_device with the optimised pose from
    the device and the PnP's d_found as written.  Equal to bow_restatement -> reloc_pnp_restatement -> pose_optimization_restatement ->
    reloc_restatement.  The candidates' points are the frame's features back-projected through the true pose where SearchByBoW's row (known
    from the restatement) matches them, 30 % of those moved away; the rest of a list lies anywhere."""
    import torch
    import bow_restatement as br
    import bow_search_cases as bc
    import local_points_restatement as lr
    import pose_optimization_cases as pc
    import pose_optimization_restatement as por
    import reloc_restatement as rr
    pkg = gpu_lib
    rng = np.random.default_rng(77)
    intr, bounds = (260.0, 260.0, 160.0, 120.0), (0.0, 320.0, 0.0, 240.0)
    sf = np.cumprod(np.concatenate([[1.0], np.full(3, 1.2)])).astype(f32)
    sigma2, inv_sigma2 = (sf * sf).astype(f32), (f32(1.0) / (sf * sf)).astype(f32)
    kfA, fr = bc.random_pair(5, 300, 250, 12)
    kfB = bc.side(np.array([bc.flip(d, 6, rng) for d in kfA["desc"]]), kfA["angles"], kfA["fv"])
    n = len(fr["desc"])
    fr["keys"]["x"], fr["keys"]["y"] = rng.uniform(15, 305, n).astype(f32), rng.uniform(15, 225, n).astype(f32)
    fr["keys"]["octave"] = rng.integers(0, 4, n)
    kps, desc = fr["keys"], fr["desc"]
    R, t = pr.rot(0.03, -0.05, 0.02), np.array([0.1, -0.05, 0.2])
    depth = rng.uniform(2.0, 8.0, n)
    Xc = np.c_[(kps["x"] - intr[2]) / intr[0] * depth, (kps["y"] - intr[3]) / intr[1] * depth, depth]
    world = ((Xc - t) @ R).astype(f32)
    cands, rows = [kfA, kfB], []
    lists = []
    for kf in cands:
        row, _ = br.search_by_bow(kf, fr, 0.75, 1)
        row = np.asarray(row, np.int32)
        pts = np.zeros(len(kf["desc"]), pkg.RELOC_POINT_DTYPE)
        pts["pos"] = rng.uniform(-4, 4, (len(pts), 3)).astype(f32) + np.array([0, 0, 5], f32)
        pts["angle"], pts["desc"], pts["min_distance"], pts["max_distance"], pts["flags"] = kf["angles"], kf["desc"], 0.5, 12.0, 2
        m = np.nonzero(row >= 0)[0]
        pts["pos"][row[m]] = world[m]
        bad = rng.choice(m, int(0.3 * len(m)), replace=False)
        pts["pos"][row[bad]] += rng.uniform(0.5, 1.5, (len(bad), 3)).astype(f32)
        pts["flags"][row[m[:3]]] |= rp.POINT_SKIP
        rows.append(row)
        lists.append(pts)
    seeds = [11, 12]
    # ---- the restatements
    want = []
    for k in range(2):
        s = rp.PnPsolver(kps, rows[k], lists[k], sigma2, intr, seeds[k])
        s.set_ransac_parameters(**rc.REFERENCE)
        r = s.iterate(5)
        assert r.has_pose and r.n_inliers >= 30, (k, r.has_pose, r.n_inliers, r.n_correspondences)
        wm, wf = rp.match_and_found(r, rows[k], len(lists[k]))
        T = r.Tcw.reshape(3, 4)
        start = pc.camera(T[:, :3], T[:, 3], *intr, 20.0)
        has_obs = (lists[k]["flags"] & 2) != 0
        p1, o1, m1 = por.pose_optimization(kps, None, wm, lists[k]["pos"], has_obs, start, inv_sigma2, np.full(n, 7, np.uint8), 1)
        rcam = rr.camera(T[:, :3], T[:, 3], *intr, th=10.0, orb_dist=100)
        sr = rr.search(kps, desc, lists[k], rcam, wf, m1, sf, bounds, pose=(p1["Tcw"], p1["Ow"]))
        print(f"candidate {k}: {r.n_correspondences} correspondences, {r.n_inliers} PnP inliers, {p1['n_inliers']} after optimisation, "
              f"{sr['n_matches']} additional")
        want.append((r, wm, wf, start, p1, o1, rcam, sr))
    assert any(w[7]["n_matches"] > 0 for w in want)
    # ---- the device
    sides = [kfA, kfB, fr]
    cap = max(len(s["desc"]) for s in sides) + 5

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    a = dict(kps=np.zeros((3, cap), pkg.KP_DTYPE), desc=np.zeros((3, cap, 32), np.uint8), counts=np.zeros(3, np.int32), n_nodes=np.zeros(3, np.int32),
             node_ids=np.zeros((3, cap), np.uint32), node_off=np.zeros((3, cap + 1), np.int32), node_idx=np.zeros((3, cap), np.int32))
    for s, sd in enumerate(sides):
        ids, off, idx = bc.csr(sd["fv"])
        m = len(sd["desc"])
        a["counts"][s], a["n_nodes"][s] = m, len(ids)
        a["kps"][s, :m], a["desc"][s, :m] = sd["keys"], sd["desc"]
        a["node_ids"][s, :len(ids)], a["node_off"][s, :len(off)], a["node_idx"][s, :len(idx)] = ids, off, idx
    d = {k: up(v) for k, v in a.items()}
    d_kf, d_f = up(np.array([0, 1], np.int32)), up(np.array([2, 2], np.int32))
    d_bow = torch.full((2, cap), 12345, dtype=torch.int32, device="cuda")
    d_bstats = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    off = np.array([0, len(lists[0]), len(lists[0]) + len(lists[1])], np.int32)
    d_pts = up(np.concatenate(lists))
    d_state = torch.zeros((2, pkg.reloc_pnp_state_bytes(cap)), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((2, 104), dtype=torch.uint8, device="cuda")
    d_inl = torch.zeros((2, cap), dtype=torch.uint8, device="cuda")
    d_match = torch.full((2, cap), -77, dtype=torch.int32, device="cuda")
    d_found = torch.full((int(off[2]),), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mt = pkg.OrbMatcher()
    mt.bow_batch_device(d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d["n_nodes"].data_ptr(), d["node_ids"].data_ptr(),
                        d["node_off"].data_ptr(), d["node_idx"].data_ptr(), d_kf.data_ptr(), d_f.data_ptr(), 2, cap, d_bow.data_ptr(), d_bstats.data_ptr(),
                        nn_ratio=0.75, check_orientation=True)
    par = [pkg.reloc_pnp_params([f32(x) for x in intr], seeds[k], reset=1, n_iterations=5, **rc.REFERENCE) for k in range(2)]
    mt.reloc_pnp_batch_device(d["kps"].data_ptr(), d["counts"].data_ptr(), 3, d_pts.data_ptr(), [2, 2], off, d_bow.data_ptr(), sigma2, par, cap,
                              d_state.data_ptr(), d_res.data_ptr(), d_inl.data_ptr(), d_match.data_ptr(), d_found.data_ptr())
    mt.sync()
    results = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.RELOC_PNP_RESULT_DTYPE)  # the host's step: bNoMore, an empty pose, the cameras
    assert all(int(results["has_pose"][k]) == 1 for k in range(2))
    cams = []
    for k in range(2):
        T = results["Tcw"][k].reshape(3, 4)
        cams.append(pc.camera(T[:, :3], T[:, 3], *intr, 20.0))
    # the pose kernel works per frame: each pair is a frame slot of its own with the lost frame's keypoints
    k2, c2 = np.zeros((2, cap), pkg.KP_DTYPE), np.array([n, n], np.int32)
    k2[:, :n] = kps
    d_k2, d_c2 = up(k2), up(c2)
    d_outlier = torch.full((2, cap), 7, dtype=torch.uint8, device="cuda")
    d_pose = torch.zeros((2, pkg.POSE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    mt.pose_optimization_batch_device(d_k2.data_ptr(), d_c2.data_ptr(), d_match.data_ptr(), d_pts.data_ptr(), off, np.array(cams, pkg.POSE_CAMERA_DTYPE), cap,
                                      inv_sigma2, d_outlier.data_ptr(), d_pose.data_ptr(), point_stride=64,
                                      flags_offset=pkg.RELOC_POINT_DTYPE.fields["flags"][1], has_obs_bit=pkg.RELOC_POINT_HAS_OBS, clear_outliers=True)
    cell = np.full((1, cap), -1, np.int32)
    cell[0, :n] = lr.grid_cells(kps, bounds)
    d_cell, d_c1 = up(cell), up(np.array([n], np.int32))
    d_start = torch.zeros((1, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_items = torch.full((1, cap), -1, dtype=torch.int32, device="cuda")
    mt.grid_build_batch_device(d_cell.data_ptr(), d_c1.data_ptr(), 1, cap, d_start.data_ptr(), d_items.data_ptr())
    d_query = torch.zeros((int(off[2]), 48), dtype=torch.uint8, device="cuda")
    d_projected = torch.zeros((int(off[2]),), dtype=torch.uint8, device="cuda")
    d_rstats = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    d_desc1 = up(a["desc"][2:3])
    mt.reloc_batch_device(d_k2.data_ptr(), d_desc1.data_ptr(), d_c1.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), 1, d_pts.data_ptr(),
                          [0, 0], off, np.array([w[6] for w in want], rr.CAMERA), cap, sf, d_query.data_ptr(), d_projected.data_ptr(),
                          d_match.data_ptr(), d_rstats.data_ptr(), bounds=bounds, d_found=d_found.data_ptr(), d_pose=d_pose.data_ptr())
    mt.sync()
    torch.cuda.synchronize()
    bow = d_bow.cpu().numpy()
    inl, match, found, outlier = d_inl.cpu().numpy(), d_match.cpu().numpy(), d_found.cpu().numpy(), d_outlier.cpu().numpy()
    poses = np.frombuffer(d_pose.cpu().numpy().tobytes(), pkg.POSE_RESULT_DTYPE)
    rstats = np.frombuffer(d_rstats.cpu().numpy().tobytes(), pkg.RELOC_STATS_DTYPE)
    mt.close()
    for k, (r, wm, wf, start, p1, o1, rcam, sr) in enumerate(want):
        assert np.array_equal(bow[k, :n], rows[k]) and (bow[k, n:] == -1).all(), k
        rc.assert_result_equal(results[k], inl[k, :n], r, f"chain candidate {k}")
        assert cams[k].tobytes() == start.tobytes()
        assert np.array_equal(found[off[k]:off[k + 1]], wf), k
        for field in ("Rt", "Tcw", "Ow", "lambda", "chi2"):
            assert pc.same_bits(poses[field][k], p1[field]), (k, field)
        for field in ("n_edges", "n_inliers", "n_inliers_with_obs", "rounds", "status"):
            assert np.array_equal(poses[field][k], p1[field]), (k, field)
        assert np.array_equal(outlier[k, :n], o1), k
        assert tuple(int(rstats[f][k]) for f in rr.STAT_FIELDS) == tuple(int(sr[f]) for f in rr.STAT_FIELDS), k
        assert np.array_equal(match[k, :n], sr["match"]) and (match[k, n:] == -1).all(), k
