"""amos_match_sim3_batch_device on the GPU against the plain-Python restatement (tests/sim3_restatement.py), compared with == on the
bytes: every field of the result record, R12 / t12 / s12 / T12, the inlier row, d_match_out where there is a Sim3, and the generator state
the carried blob begins with -- over the calls of every case of tests/sim3_cases.py on carried state, a reset, a batch of eight pairs over
three keyframe slots with a disabled pair, the status bits, a restart on a state of another N, the 2049-correspondence refusal, the
argument errors, and the chain SearchByBoW(KF, KF) row -> Sim3 on resident arrays.  Outputs are pre-filled with a pad pattern so that
"not written" is visible; the state is pre-filled with garbage before a reset."""
import numpy as np
import pytest

import sim3_cases as sc
import sim3_restatement as sr

pytestmark = pytest.mark.gpu
f32 = np.float32
PAD = 0x5A  # what the outputs hold on entry
# the carried blob, for the two white-box reads below: generator (8 bytes), magic, N, minInliers, fixScale, maxIts, iterations, bestInliers,
# then the best R [9], t [3], s, T12 [16] and the best inlier mask by correspondence index
STATE_BEST, STATE_MASK = 36, 36 + 29 * 4


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Resident:
    """Keyframes and pairs uploaded once; every run() is one amos_match_sim3_batch_device call on the same carried state."""

    def __init__(self, pkg, frames, pairs, cap=sc.CAPACITY, matcher=None, d_match12=None, level_sigma2=sc.LEVEL_SIGMA2):
        """frames: list of dict(kps, points, cam); pairs: list of dict(f1, f2, match12 [n of frame f1])."""
        import torch
        self.torch, self.pkg, self.cap, self.pairs, self.frames, self.sigma2 = torch, pkg, cap, pairs, frames, level_sigma2
        nf, npairs = len(frames), len(pairs)
        kps, counts = np.zeros((nf, cap), pkg.KP_DTYPE), np.zeros(nf, np.int32)
        kps["octave"] = 99  # padding that must not be read
        points = np.zeros((nf, cap), pkg.SIM3_POINT_DTYPE)
        self.cameras = np.zeros(nf, pkg.SIM3_CAMERA_DTYPE)
        for f, fr in enumerate(frames):
            n = len(fr["kps"])
            counts[f] = n
            kps[f, :n], points[f, :n] = fr["kps"], fr["points"]
            for name in pkg.SIM3_CAMERA_DTYPE.names:
                self.cameras[name][f] = fr["cam"][name]
        rows = np.full((npairs, cap), 123456, np.int32)  # a row's padding names no feature of keyframe 2
        for k, p in enumerate(pairs):
            rows[k, :len(p["match12"])] = p["match12"]
        self.d_kps, self.d_counts, self.d_points = up(kps), up(counts), up(points)
        self.d_match12 = up(rows) if d_match12 is None else d_match12
        self.d_p1, self.d_p2 = up(np.array([p["f1"] for p in pairs], np.int32)), up(np.array([p["f2"] for p in pairs], np.int32))
        self.state_bytes = pkg.sim3_state_bytes(cap)
        self.d_state = torch.full((npairs, self.state_bytes), 0xCD, dtype=torch.uint8, device="cuda")  # garbage: a reset must not read it
        self.mt = matcher or pkg.OrbMatcher()
        self.own = matcher is None

    def run(self, params):
        """-> (results [pairs], inlier [pairs][cap], match_out [pairs][cap], generator states [pairs])"""
        torch, pkg, npairs, cap = self.torch, self.pkg, len(self.pairs), self.cap
        self.d_result = torch.full((npairs, 160), PAD, dtype=torch.uint8, device="cuda")
        self.d_inlier = torch.full((npairs, cap), PAD, dtype=torch.uint8, device="cuda")
        self.d_out = torch.full((npairs, cap), -77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.mt.sim3_batch_device(self.d_kps.data_ptr(), self.d_counts.data_ptr(), self.d_points.data_ptr(), self.cameras, self.d_p1.data_ptr(),
                                  self.d_p2.data_ptr(), npairs, self.d_match12.data_ptr(), self.sigma2, params, cap, self.d_state.data_ptr(),
                                  self.d_result.data_ptr(), self.d_inlier.data_ptr(), self.d_out.data_ptr())
        self.mt.sync()
        torch.cuda.synchronize()
        results = np.frombuffer(self.d_result.cpu().numpy().tobytes(), pkg.SIM3_RESULT_DTYPE)
        self.state = self.d_state.cpu().numpy()
        states = np.frombuffer(self.state[:, :8].tobytes(), np.uint64)
        return results, self.d_inlier.cpu().numpy(), self.d_out.cpu().numpy(), states

    def restatement(self, k, seed, fix_scale=0, params=sc.REFERENCE, trace=False):
        p = self.pairs[k]
        a, b = self.frames[p["f1"]], self.frames[p["f2"]]
        s = sr.Sim3Solver(a["kps"], a["points"], a["cam"], b["kps"], b["points"], b["cam"], p["match12"], self.sigma2, fix_scale=fix_scale, seed=seed,
                          trace=trace)
        s.set_ransac_parameters(**params)
        return s

    def close(self):
        if self.own:
            self.mt.close()


def frames_of(pair):
    return [dict(kps=pair["kps1"], points=pair["points1"], cam=pair["cam1"]), dict(kps=pair["kps2"], points=pair["points2"], cam=pair["cam2"])]


def params_of(pkg, c, reset, **kw):
    return pkg.sim3_params(c["seed"], reset=reset, n_iterations=c["n_iterations"], fix_scale=c["fix_scale"], **dict(c["params"], **kw))


def assert_pair(got, k, res, want, rng_state, what):
    """pair k of one device call against the restatement's Result: record, rows, paddings, match_out."""
    results, inlier, out, states = got
    n, cap = len(res.frames[res.pairs[k]["f1"]]["kps"]), res.cap
    print(what, {f: int(results[f][k]) for f in sc.RESULT_FIELDS})
    sc.assert_result_equal(results[k], inlier[k, :n], want, what)
    assert int(results["skipped"][k]) == 0
    assert not inlier[k, n:].any(), f"{what}: inlier padding"
    if want.has_sim3:
        assert np.array_equal(out[k, :n], want.match_out) and (out[k, n:] == -1).all(), f"{what}: d_match_out"
    else:
        assert (out[k] == -77).all(), f"{what}: d_match_out written without a Sim3"
    if rng_state is not None:
        assert int(states[k]) == rng_state, f"{what}: generator state"


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_calls_on_carried_state_equal_the_restatement(gpu_lib, name):
    pair, c, want, s = sc.case(name)
    res = Resident(gpu_lib, frames_of(pair), [dict(f1=0, f2=1, match12=pair["match12"])])
    for call, (w, rng) in enumerate(want):
        got = res.run([params_of(gpu_lib, c, reset=1 if call == 0 else 0)])
        assert_pair(got, 0, res, w, rng, f"{name} call {call}")
    if s.best is not None:  # the best set behind the last call, Sim3 or not: the LAST of equal maxima (white box: the blob's layout)
        best = np.frombuffer(res.state[0, STATE_BEST:STATE_MASK].tobytes(), f32)
        wantbest = np.concatenate([s.best.R.reshape(9), s.best.t, [s.best.s], s.best.T12.reshape(16)]).astype(f32)
        assert best.tobytes() == wantbest.tobytes(), f"{name}: the carried best Sim3"
        mask = np.unpackbits(res.state[0, STATE_MASK:STATE_MASK + 256], bitorder="little")[:s.N].astype(bool)
        assert np.array_equal(mask, s.best_mask), f"{name}: the carried best set"
    # reset = 1 reproduces the first call
    got = res.run([params_of(gpu_lib, c, reset=1)])
    assert_pair(got, 0, res, want[0][0], want[0][1], f"{name} after reset")
    res.close()


SLOT_CAMERAS = [sc.camera(sc.rotation((0.1, 0.9, 0.3), 0.4), np.array([0.2, -0.3, 0.5]), sc.K1),
                sc.camera(sc.rotation((-0.5, 0.2, 0.7), -0.3), np.array([-0.4, 0.1, 0.3]), sc.K2),
                sc.camera(sc.rotation((0.6, 0.1, -0.4), 0.2), np.array([0.1, 0.2, -0.2]), (535.4, 539.2, 320.1, 247.6))]


def batch_of_eight():
    """Eight pairs over three keyframe slots; every slot holds the features of its pairs' scenes, a pair's row names only its own."""
    slots = [(0, 1), (0, 2), (1, 2), (1, 0), (2, 0), (2, 1), (0, 1), (1, 2)]
    spec = [(60, 0.4, 0.5), (24, 0.0, 0.5), (40, 0.4, 0.5), (48, 0.3, 0.5), (30, 0.2, 0.0), (60, 0.75, 0.0), (36, 0.4, 1.0), (19, 0.0, 0.0)]
    sides = [[], [], []]
    scenes = []
    for k, ((f1, f2), (nc, out, noise)) in enumerate(zip(slots, spec)):
        pair = sc.make_pair(nc, out, noise, 100 + k, cams=(SLOT_CAMERAS[f1], SLOT_CAMERAS[f2]), fix_scale=k % 2)
        base1, base2 = sum(len(x[0]) for x in sides[f1]), sum(len(x[0]) for x in sides[f2])
        sides[f1].append((pair["kps1"], pair["points1"]))
        base2 += len(pair["kps1"]) if f1 == f2 else 0
        sides[f2].append((pair["kps2"], pair["points2"]))
        scenes.append((base1, base2, pair["match12"]))
    frames = [dict(kps=np.concatenate([x[0] for x in sd]), points=np.concatenate([x[1] for x in sd]), cam=SLOT_CAMERAS[f]) for f, sd in enumerate(sides)]
    pairs = []
    for (f1, f2), (base1, base2, m12) in zip(slots, scenes):
        row = np.full(len(frames[f1]["kps"]), -1, np.int32)
        row[base1:base1 + len(m12)] = np.where(m12 >= 0, m12 + base2, -1)
        pairs.append(dict(f1=f1, f2=f2, match12=row))
    return frames, pairs


def test_batch_of_eight_pairs_over_three_slots_with_a_disabled_pair(gpu_lib):
    frames, pairs = batch_of_eight()
    cap = max(len(f["kps"]) for f in frames) + 7
    res = Resident(gpu_lib, frames, pairs, cap=cap)
    disabled = 3
    wants = []
    for k in range(8):
        s = res.restatement(k, 1000 + k, fix_scale=k % 2)
        wants.append([(s.iterate(sc.N_ITERATIONS), s.rng.s) for _ in range(3)])

    def params(call, ks=range(8)):
        return [gpu_lib.sim3_params(1000 + k, reset=1 if call == 0 else 0, n_iterations=sc.N_ITERATIONS, fix_scale=k % 2, enabled=0 if k == disabled else 1,
                                    **sc.REFERENCE) for k in ks]
    seen = []
    for call in range(3):
        got = res.run(params(call))
        seen.append(got)
        for k in range(8):
            if k == disabled:
                rec = got[0][k]
                assert int(rec["skipped"]) == 1 and not np.frombuffer(rec.tobytes(), np.uint8)[:-4].any()
                assert (got[1][k] == PAD).all() and (got[2][k] == -77).all() and (res.state[k] == 0xCD).all(), "a disabled pair writes its record only"
                continue
            w, rng = wants[k][call]
            assert_pair(got, k, res, w, rng, f"call {call} pair {k}")
    assert sum(int(w.has_sim3) for ws in wants for w, _ in ws) >= 4
    # one pair run alone gives the same bytes as in the batch
    k = 5
    single = Resident(gpu_lib, frames, [pairs[k]], cap=cap, matcher=res.mt)
    for call in range(3):
        got = single.run(params(call, [k]))
        for a, b in zip(got, seen[call]):
            assert a[0].tobytes() == b[k].tobytes(), f"pair {k} alone, call {call}"
    res.close()


def test_status_bits_restart_and_slot_check(gpu_lib):
    pair, c, _, _ = sc.case("three_calls")
    pair = dict(pair, kps1=pair["kps1"].copy(), kps2=pair["kps2"].copy(), match12=pair["match12"].copy())
    good = pair["good1"]
    pair["kps1"]["octave"][good[3]] = 8
    pair["kps2"]["octave"][pair["match12"][good[4]]] = -1
    pair["match12"][good[5]] = sc.N_FEATURES
    other, c2, want2, _ = sc.case("n24")
    frames = frames_of(pair) + frames_of(other)
    pairs = [dict(f1=0, f2=1, match12=pair["match12"]), dict(f1=2, f2=3, match12=other["match12"]), dict(f1=0, f2=4, match12=pair["match12"])]
    res = Resident(gpu_lib, frames, pairs)
    s = res.restatement(0, c["seed"])
    assert s.status == 3 and s.N == c["nc"] - 3
    got = res.run([params_of(gpu_lib, c, 1), params_of(gpu_lib, c2, 1), params_of(gpu_lib, c, 1)])
    assert_pair(got, 0, res, s.iterate(sc.N_ITERATIONS), s.rng.s, "status bits")
    assert_pair(got, 1, res, want2[0][0], want2[0][1], "n24 beside it")
    rec = got[0][2]  # keyframe-2 slot 4 of 4 frames
    assert int(rec["code"]) == -4 and not np.frombuffer(rec.tobytes(), np.uint8)[116 + 4:].any() and (got[1][2] == PAD).all() and (got[2][2] == -77).all()
    # pair 1's state now is a solver of 24 correspondences: pair 0's inputs on it start over and say so
    res2 = Resident(gpu_lib, frames, [pairs[0]], matcher=res.mt)
    res2.d_state[0].copy_(res.d_state[1])
    s = res.restatement(0, 4242)
    w = s.iterate(sc.N_ITERATIONS)
    w.status |= 4
    got = res2.run([gpu_lib.sim3_params(4242, reset=0, **sc.REFERENCE)])
    assert_pair(got, 0, res2, w, s.rng.s, "restart on a state of another N")
    w = s.iterate(sc.N_ITERATIONS)  # and the next call goes on from it
    got = res2.run([gpu_lib.sim3_params(4242, reset=0, **sc.REFERENCE)])
    assert_pair(got, 0, res2, w, s.rng.s, "the call after the restart")
    res.close()


def test_2049_correspondences_are_refused_with_nothing_else_written(gpu_lib):
    big = sc.make_pair(2049, 0.0, 0.0, 11, n_features=4096, skipped=0)
    res = Resident(gpu_lib, frames_of(big), [dict(f1=0, f2=1, match12=big["match12"])], cap=4096)
    got = res.run([gpu_lib.sim3_params(1, **sc.REFERENCE)])
    rec = got[0][0]
    assert int(rec["code"]) == -3 and int(rec["n_correspondences"]) == 2049 and int(rec["has_sim3"]) == 0 and int(rec["status"]) == 0
    assert (got[1] == PAD).all() and (got[2] == -77).all() and (res.state == 0xCD).all()
    # 2048 of them run
    ok = sc.make_pair(2048, 0.0, 0.0, 12, n_features=4096, skipped=0)
    res2 = Resident(gpu_lib, frames_of(ok), [dict(f1=0, f2=1, match12=ok["match12"])], cap=4096, matcher=res.mt)
    s = res2.restatement(0, 1)
    got = res2.run([gpu_lib.sim3_params(1, **sc.REFERENCE)])
    assert_pair(got, 0, res2, s.iterate(sc.N_ITERATIONS), s.rng.s, "2048 correspondences")
    res.close()


def test_argument_errors(gpu_lib):
    pair, c, _, _ = sc.case("n24")
    res = Resident(gpu_lib, frames_of(pair), [dict(f1=0, f2=1, match12=pair["match12"])])
    good = params_of(gpu_lib, c, 1)
    res.run([good])
    for kw in (dict(probability=0.0), dict(probability=1.0), dict(min_inliers=2), dict(max_iterations=0), dict(max_iterations=65537)):
        with pytest.raises(gpu_lib.AmosError):
            res.run([params_of(gpu_lib, c, 1, **kw)])
    for n_it in (0, 65537):
        with pytest.raises(gpu_lib.AmosError):
            res.run([gpu_lib.sim3_params(1, n_iterations=n_it, **sc.REFERENCE)])
    res.cameras["tcw"][1, 2] = np.nan
    with pytest.raises(gpu_lib.AmosError):
        res.run([good])
    res.cameras["tcw"][1, 2] = 0.0
    saved, res.d_match12 = res.d_match12, None

    class Null:
        def data_ptr(self):
            return None
    res.d_match12 = Null()
    with pytest.raises(gpu_lib.AmosError):
        res.run([good])
    res.d_match12 = saved
    saved, res.sigma2 = res.sigma2, np.ones(17, f32)
    with pytest.raises(gpu_lib.AmosError):
        res.run([good])
    res.sigma2 = saved
    res.run([good])  # the handle still works
    res.close()


def test_chain_bow_search_then_sim3_on_resident_arrays(gpu_lib):
    """amos_match_bow_kf_batch_device writes d_match12 for four candidate pairs, amos_match_sim3_batch_device reads it in place: no host
    round trip in between.  The map points obey one similarity per scene along the ORACLE's matches (orc_search_by_bow_kf), so the device's
    d_match_out is held to what the restatement makes of the oracle's row."""
    import torch
    import kf_search_cases as kc
    pkg = gpu_lib
    sides, pairs_idx = [], [(0, 1), (1, 0), (2, 3), (3, 2)]
    for seed in (5, 6):
        k1, k2, _, _ = kc.random_pair(seed, point_share=0.9)
        sides += [k1, k2]
    rows = [kc.oracle_bow_kf(sides[a], sides[b], 0.75, 1)[1] for a, b in pairs_idx]
    rng = np.random.default_rng(77)
    s, R, t = sc.TRUTH
    frames = []
    for f, sd in enumerate(sides):
        n = len(sd["desc"])
        pts = np.zeros(n, sc.POINT)
        pts["flags"] = np.where(sd["has_point"] != 0, 0, sr.POINT_SKIP)
        frames.append(dict(kps=sd["keys"], points=pts, cam=SLOT_CAMERAS[f % 3], Xc=None))
    for (a, b), row in list(zip(pairs_idx, rows))[::2]:  # X_a = s R X_b + t along the oracle's matches of (a, b); the rest anywhere in front
        na, nb = len(sides[a]["desc"]), len(sides[b]["desc"])
        z = rng.uniform(2.0, 8.0, na)
        Xa = np.stack([rng.uniform(-0.3, 0.3, na) * z, rng.uniform(-0.25, 0.25, na) * z, z], 1)
        zb = rng.uniform(2.0, 8.0, nb)
        Xb = np.stack([rng.uniform(-0.3, 0.3, nb) * zb, rng.uniform(-0.25, 0.25, nb) * zb, zb], 1)
        m = np.nonzero(row >= 0)[0]
        Xb[row[m]] = (Xa[m] - t) @ R / s
        for f, X in ((a, Xa), (b, Xb)):
            cam = frames[f]["cam"]
            Rc, tc = cam["Rcw"].reshape(3, 3).astype(np.float64), cam["tcw"].astype(np.float64)
            frames[f]["points"]["pos"] = (X - tc) @ Rc
    cap = max(len(sd["desc"]) for sd in sides) + 5
    d = {k: up(v) for k, v in kc.pack(sides, cap, 1).items()}
    d_1, d_2 = up(np.array([p[0] for p in pairs_idx], np.int32)), up(np.array([p[1] for p in pairs_idx], np.int32))
    d_match = torch.full((4, cap), 12345, dtype=torch.int32, device="cuda")
    d_stats = torch.full((4, 4), -9, dtype=torch.int32, device="cuda")
    res = Resident(pkg, frames, [dict(f1=a, f2=b, match12=row) for (a, b), row in zip(pairs_idx, rows)], cap=cap, d_match12=d_match)
    res.d_p1, res.d_p2 = d_1, d_2
    params = dict(sc.REFERENCE, min_inliers=12)
    torch.cuda.synchronize()
    res.mt.bow_kf_batch_device(d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d["n_nodes"].data_ptr(), d["node_ids"].data_ptr(),
                               d["node_off"].data_ptr(), d["node_idx"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(), 4, cap, d_match.data_ptr(),
                               d_stats.data_ptr(), nn_ratio=0.75, check_orientation=1, d_has_point=d["has_point"].data_ptr())
    got = res.run([pkg.sim3_params(500 + k, n_iterations=300, **params) for k in range(4)])  # find(): the same stream, no synchronisation between
    n_sim3 = 0
    for k in range(4):
        sol = res.restatement(k, 500 + k, params=params)
        w = sol.iterate(300)
        assert_pair(got, k, res, w, sol.rng.s, f"chain pair {k}")
        n_sim3 += w.has_sim3
    assert n_sim3 >= 2, "the chain's scenes are meant to close"
    res.close()
