"""CPU: constants the reference itself pins (SURVEY.md 8c "known-answer material"), and the C-ABI
library's export table."""
import ctypes
import hashlib
import os
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pattern_from_header():
    src = open(os.path.join(ROOT, "include", "amos_orb_pattern.h")).read()
    body = src[src.index("amos_orb_pattern[256 * 4] = {"):]
    body = body[body.index("{") + 1:body.index("};")]
    return [int(x) for x in re.findall(r"-?\d+", body)]


def test_bit_pattern_sha256():
    """bit_pattern_31_ (ORBextractor.cc:231-489) as int32-LE, sha256 from SURVEY.md Appendix B."""
    nums = _pattern_from_header()
    assert len(nums) == 1024
    digest = hashlib.sha256(struct.pack("<1024i", *nums)).hexdigest()
    assert digest == "7e645581387b82784797e8adddb9b6f0c12611859fda09ca8a9bec96d767a05f"
    assert nums[:8] == [8, -3, 9, 5, 4, 2, 7, -12]  # first two pairs, ORBextractor.cc:233-234
    assert max(abs(v) for v in nums) == 13


def test_ctor_tables(ob):
    """umax, per-level quotas and level sizes at the TUM parameters (TUM1.yaml / SURVEY section 8)."""
    t = ob.Oracle(1000, 1.2, 8, 20, 7).tables()
    assert list(t["umax"]) == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    assert list(t["features_per_level"]) == [217, 181, 151, 126, 105, 87, 73, 60]
    assert t["scale"][0] == 1.0 and t["scale"][1] == np.float32(1.2)
    assert t["scale"][2] == np.float32(1.2) * np.float32(1.2)
    assert np.array_equal(t["sigma2"], t["scale"] * t["scale"])
    lw, lh = ob.Oracle(1000, 1.2, 8).level_sizes(640, 480)
    assert list(lw) == [640, 533, 444, 370, 309, 257, 214, 179]
    assert list(lh) == [480, 400, 333, 278, 231, 193, 161, 134]
    t5 = ob.Oracle(4000, 1.2, 12, 20, 7).tables()
    assert list(t5["features_per_level"]) == [751, 626, 521, 435, 362, 302, 251, 210, 175, 146, 121, 100]
    lw, lh = ob.Oracle(4000, 1.2, 12).level_sizes(1920, 1080)
    assert list(lw) == [1920, 1600, 1333, 1111, 926, 772, 643, 536, 447, 372, 310, 258]
    assert list(lh) == [1080, 900, 750, 625, 521, 434, 362, 301, 251, 209, 174, 145]


def test_thresholds(pkg):
    assert (pkg.TH_HIGH, pkg.TH_LOW, pkg.HISTO_LENGTH) == (100, 50, 30)  # ORBmatcher.cc:49-51
    hdr = open(os.path.join(ROOT, "include", "amos_frontend.h")).read()
    assert "#define AMOS_TH_HIGH 100" in hdr and "#define AMOS_TH_LOW 50" in hdr and "#define AMOS_HISTO_LENGTH 30" in hdr
    assert "#define AMOS_EDGE_THRESHOLD 19" in hdr


def test_cabi_exports_every_declared_symbol(pkg):
    """The shared library loads without a GPU and exports every function include/*.h declares."""
    hdr = open(os.path.join(ROOT, "include", "amos_frontend.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(amos_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 30
    assert os.path.exists(pkg.LIB_PATH), "build libamos_frontend.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(pkg.LIB_PATH)
    missing = [n for n in declared if not hasattr(lib, n)]
    assert not missing, missing
    assert sorted(pkg.EXPORTS) == declared


def test_prototype_table_matches_the_header(pkg):
    """The binding's one table of prototypes against include/amos_frontend.h: for every declared function the number of argtypes is the
    number of parameters, the restype is the declared return type, every pointer parameter is a void pointer and every scalar its own type."""
    hdr = open(os.path.join(ROOT, "include", "amos_frontend.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = re.findall(r"([A-Za-z_][\w \*]*?)\b(amos_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)
    assert sorted(name for _, name, _ in protos) == sorted(set(re.findall(r"\b(amos_[a-z0-9_]+)\s*\(", hdr)))  # every declaration parsed
    restypes = {"void": None, "void *": ctypes.c_void_p, "const char *": ctypes.c_char_p, "size_t": ctypes.c_size_t, "int": ctypes.c_int}
    scalars = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
               "long long": ctypes.c_longlong, "uint32_t": ctypes.c_uint32}
    assert sorted(pkg.PROTOTYPES) == sorted(name for _, name, _ in protos)
    for ret, name, params in protos:
        params = [p for p in (q.strip() for q in params.split(",")) if p and p != "void"]
        restype, argtypes = pkg.PROTOTYPES[name]
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        assert restype is restypes[" ".join(ret.split())], (name, ret, restype)
        for p, t in zip(params, argtypes):  # a pointer is a void pointer, a scalar its own type
            want = ctypes.c_void_p if "*" in p or "[" in p else scalars[" ".join(p.replace("const ", "").split()[:-1])]
            assert t is want, (name, p, t)
    L = pkg.lib()  # applied once, to every function
    for name, (restype, argtypes) in pkg.PROTOTYPES.items():
        assert getattr(L, name).restype is restype and tuple(getattr(L, name).argtypes) == tuple(argtypes), name


def test_keypoint_layout_matches_cv_keypoint(pkg):
    """amos_keypoint must be memcpy-compatible with cv::KeyPoint (7 x 4 bytes, pt first)."""
    assert pkg.KP_DTYPE.itemsize == 28
    assert pkg.KP_DTYPE.names == ("x", "y", "size", "angle", "response", "octave", "class_id")
    assert pkg.BEST2_DTYPE.itemsize == 16


def test_missing_library_fails_loudly(pkg, tmp_path, monkeypatch):
    """No CPU fallback: without the HIP extension the binding raises."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("amos_slam_amd_probe", os.path.join(ROOT, "amos-slam_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.LIB_PATH = str(tmp_path / "nope.so")
    try:
        mod.lib()
    except mod.AmosError as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("lib() must raise when the extension is missing")


def test_product_never_touches_the_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline leg may build, load or call oracle/."""
    needles = ("orb_oracle", "liborb_oracle", "oracle/", "oracle_binding", "orc_")
    for top in ("amos-slam_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".so", ".o", ".pyc")):
                    continue
                text = open(os.path.join(dirpath, f), errors="replace").read()
                hits = [n for n in needles if n in text]
                assert not hits, (dirpath, f, hits)
