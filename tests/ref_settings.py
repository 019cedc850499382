"""The reference's settings files (tests/golden/ref_settings/{Monocular,RGB-D,Stereo}/*.yaml, byte-for-byte copies) read the way Tracking.cc
reads them: every number a float32 (`float fx = fSettings["Camera.fx"]`), the distortion list four entries long unless the file has a
`Camera.k3` (Tracking.cc resizes DistCoef to 5 only then).  TEST INFRASTRUCTURE ONLY.  The reader takes the `key: value` lines and needs
no YAML package; the `%YAML:1.0` header, comments and the `!!opencv-matrix` blocks (EuRoC's LEFT.* / RIGHT.* rectification) are skipped.
Also the cameras whose image bounds the projection-window search tests run at, with their keypoints undistorted by the CPU oracle."""
import collections
import os
import re

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_settings")
SENSORS = ("Monocular", "RGB-D", "Stereo")
# the Monocular files carry no frame size: the data sets' own
MONO_SIZES = {"TUM": (640, 480), "EuRoC": (752, 480), "KITTI": (1241, 376)}
f32 = np.float32

Settings = collections.namedtuple("Settings", "sensor name width height fx fy cx cy dist bf th_depth depth_map_factor n_features scale_factor "
                                              "n_levels ini_th min_th")
_LINE = re.compile(r"^([A-Za-z][\w.]*)\s*:\s*([^\s#]+)")


def files():
    """[(sensor, name)] of every settings file, sorted."""
    return [(s, f[:-5]) for s in SENSORS for f in sorted(os.listdir(os.path.join(ROOT, s))) if f.endswith(".yaml")]


def raw(sensor, name):
    """key -> float32 for the scalar `key: value` lines at column 0 (the members of a matrix block are indented, its head has no number)."""
    out = {}
    with open(os.path.join(ROOT, sensor, name + ".yaml"), encoding="utf-8") as fh:
        for line in fh:
            m = _LINE.match(line)
            if not m or m.group(2).startswith("!!"):
                continue
            try:
                out[m.group(1)] = f32(m.group(2))
            except ValueError:
                pass
    return out


def read(sensor, name):
    r = raw(sensor, name)
    if "Camera.width" in r:
        width, height = int(r["Camera.width"]), int(r["Camera.height"])
    else:
        width, height = next(size for prefix, size in MONO_SIZES.items() if name.startswith(prefix))
    dist = [r["Camera.k1"], r["Camera.k2"], r["Camera.p1"], r["Camera.p2"]] + ([r["Camera.k3"]] if "Camera.k3" in r else [])
    return Settings(sensor, name, width, height, r["Camera.fx"], r["Camera.fy"], r["Camera.cx"], r["Camera.cy"], tuple(dist), r.get("Camera.bf"),
                    r.get("ThDepth"), r.get("DepthMapFactor"), int(r["ORBextractor.nFeatures"]), r["ORBextractor.scaleFactor"],
                    int(r["ORBextractor.nLevels"]), int(r["ORBextractor.iniThFAST"]), int(r["ORBextractor.minThFAST"]))


def kernel_key(s):
    """What the kernels of a sensor's front end are given: frame size, intrinsics, coefficients and ORB parameters always; bf for the depth
    and stereo glue; the depth factor for RGB-D only.  ThDepth and the viewer's values reach no kernel."""
    key = (s.sensor, s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.dist, s.n_features, s.scale_factor, s.n_levels, s.ini_th, s.min_th)
    if s.sensor != "Monocular":
        key += (s.bf,)
    if s.sensor == "RGB-D":
        key += (s.depth_map_factor,)
    return tuple(float(v) if isinstance(v, np.floating) else v for v in key)


def cases():
    """One Settings per distinct kernel_key, in file order (the first file of a group stands for it)."""
    seen, out = set(), []
    for sensor, name in files():
        s = read(sensor, name)
        if kernel_key(s) not in seen:
            seen.add(kernel_key(s))
            out.append(s)
    return out


def case_id(s):
    return f"{s.sensor}-{s.name}"


def intrinsics(s):
    return float(s.fx), float(s.fy), float(s.cx), float(s.cy)


def dist_array(s):
    return np.array(s.dist, f32)


def orb_kwargs(s):
    return dict(n_features=s.n_features, scale_factor=float(s.scale_factor), n_levels=s.n_levels, ini_th=s.ini_th, min_th=s.min_th)


def inv_depth_factor(s):
    """mDepthMapFactor as Tracking.cc:145-149 leaves it: 1 below 1e-5, else 1.0f / factor."""
    return 1.0 if abs(float(s.depth_map_factor)) < 1e-5 else float(f32(1.0) / s.depth_map_factor)


# ---------------------------------------------------------------------------------------------------------------- the searches' cameras

# bounds that are neither zero-based nor round: TUM1's lie inside the image, Bonn's and EuRoC's (negative k1) outside
SEARCH_CAMERAS = {"TUM1": ("RGB-D", "TUM1"), "Bonn": ("RGB-D", "Bonn"), "EuRoC": ("Monocular", "EuRoC")}
IMAGE_BOUNDS_SIGN = {"TUM1": 1, "Bonn": -1, "EuRoC": -1}  # of min_x and min_y


def search_camera(ob, name):
    """dict(w, h, intr, dist, bounds) of one of SEARCH_CAMERAS, the bounds from the CPU oracle's ComputeImageBounds."""
    s = read(*SEARCH_CAMERAS[name])
    bounds = ob.image_bounds(s.width, s.height, *intrinsics(s), dist_array(s))
    sign = IMAGE_BOUNDS_SIGN[name]
    assert bounds[0] * sign > 0 and bounds[2] * sign > 0, (name, bounds)
    assert bounds != (0.0, float(s.width), 0.0, float(s.height))
    return dict(w=s.width, h=s.height, intr=intrinsics(s), dist=dist_array(s), bounds=bounds, settings=s)


def undistorted(ob, kps, cam):
    """mvKeysUn: the keypoints with x, y through the oracle's cv::undistortPoints (Frame.cc:1052-1118)."""
    out = kps.copy()
    if len(kps):
        xy = ob.undistort_points(np.stack([kps["x"], kps["y"]], 1), *cam["intr"], cam["dist"])
        out["x"], out["y"] = xy[:, 0], xy[:, 1]
    return out


def camera_scene(ob, synth, name, n_frames=2, stream=3):
    """A scene entry for the search tests at a camera's bounds: frames of the camera's size extracted by the oracle with the file's ORB
    parameters, the keypoints undistorted with the camera.  -> dict(frames [(kps_un, desc)], sf, bounds, nl, intr, image_bounds)."""
    cam = search_camera(ob, name)
    s = cam["settings"]
    orc = ob.Oracle(**orb_kwargs(s))
    frames = []
    for k in range(n_frames):
        kps, desc = orc.extract(synth.frame(stream, k, cam["h"], cam["w"]))
        frames.append((undistorted(ob, kps, cam), desc))
    return dict(frames=frames, sf=orc.tables()["scale"], bounds=cam["bounds"], nl=s.n_levels, intr=cam["intr"],
                image_bounds=(0.0, float(cam["w"]), 0.0, float(cam["h"])))


def move_into_the_sliver(points, Rcw, tcw, intr, bounds, image_bounds, n=8):
    """Makes a scene tell a camera's bounds from (0, w, 0, h): of the 2n points (records with a "pos" field, any of the searches') that
    project nearest the left border, inside both rectangles and in front of the camera, every other one is moved sideways onto u = half
    way between the camera's min_x and 0 -- inside exactly one of the two rectangles -- and the others 10 px left of both, where the
    bounds test fails whichever rectangle is used; their v and their distance to the camera centre (which the
    searches' distance gates read) stay.  Changes `points` in place, -> the indices moved."""
    fx, fy, cx, cy = intr
    R, t = np.asarray(Rcw, np.float64).reshape(3, 3), np.asarray(tcw, np.float64)
    Pc = points["pos"].astype(np.float64) @ R.T + t
    with np.errstate(all="ignore"):
        u, v = fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy
    ok = (Pc[:, 2] > 0) & (u > max(bounds[0], image_bounds[0])) & (u < min(bounds[1], image_bounds[1]))
    ok &= (v > max(bounds[2], image_bounds[2]) + 1) & (v < min(bounds[3], image_bounds[3]) - 1)
    idx = np.nonzero(ok)[0]
    idx = idx[np.argsort(u[idx], kind="stable")[:2 * n]]
    target = np.where(np.arange(len(idx)) % 2 == 0, 0.5 * (bounds[0] + image_bounds[0]), min(bounds[0], image_bounds[0]) - 10.0)
    ray = np.stack([(target - cx) / fx, (v[idx] - cy) / fy, np.ones(len(idx))], 1)
    moved = ray * (np.linalg.norm(Pc[idx], axis=1) / np.linalg.norm(ray, axis=1))[:, None]
    points["pos"][idx] = ((moved - t) @ R).astype(f32)  # R^T (Pc - t)
    return idx
