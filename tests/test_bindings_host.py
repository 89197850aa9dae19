"""The Python bindings as far as they can be checked without the libraries' code: ``HipCtx`` and ``Localizer`` are made with
``__new__`` and given a recording stand-in for the loaded library, so every shared method shows which symbol it calls, that the
handle goes first, what comes back when the call answers 0 and what is raised when it answers FLIMO_ERR_INVALID (-2).  With the
libraries loaded: every function the three headers declare has ``argtypes``, both symbols of a paired row take the same arguments,
and a shared method is ONE function on both classes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fast_limo_amd import _abi, _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SIZES = ("flimo_map_size", "flimo_loc_map_size", "flimo_scan_size", "flimo_desc_ref_size", "flimo_loc_ctx")


class _Recorder:
    """Stands in for a loaded library: every attribute is a callable that notes (symbol, arguments) and returns ``rc``;
    flimo_last_error returns bytes, the size getters (and flimo_loc_ctx: a null handle) return 0."""

    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "flimo_last_error":
                return b"said the library"
            return 0 if name in _SIZES else self.rc
        return fn


def _hip_ctx(rc):
    ctx = _lib.HipCtx.__new__(_lib.HipCtx)
    ctx._L, ctx._h = _Recorder(rc), C.c_void_p(0x1000)
    return ctx


def _localizer(rc):
    loc = api.Localizer.__new__(api.Localizer)
    loc._L, loc._h = _Recorder(rc), C.c_void_p(0x2000)
    loc.hip = api._MapperCtxView.__new__(api._MapperCtxView)
    loc.hip._loc, loc.hip._L, loc.hip.close = loc, _Recorder(0), lambda: None
    return loc


def _shape(v):
    """What a result is made of: dicts and tuples by their parts, arrays as "dtype:ndim", everything else by its type's name."""
    if isinstance(v, dict):
        return {k: _shape(x) for k, x in v.items()}
    if isinstance(v, tuple):
        return tuple(_shape(x) for x in v)
    if isinstance(v, np.ndarray):
        return f"{v.dtype}:{v.ndim}"
    return type(v).__name__


def _ints(*names):
    return {name: "int" for name in names}


_OUTLIER_STATS = dict(_ints("n", "n_stat"), mu="float", sigma="float", threshold="float", **_ints("few", "far", "outliers"))
_CLUSTER_STATS = _ints("n", "clusters", "largest", "sel_clusters", "sel_points")
_VOXEL_STATS = _ints("n", "voxels", "largest", "outside", "sel_points")
_REGION_STATS = _ints("n", "smooth", "regions", "largest", "sel_regions", "unassigned", "sel_points")
_NORMALS = {"normal": "float32:2", "cnt": "int32:1", "centroid": "float64:2", "cov": "float64:2", "eig": "float64:2"}
_X26, _XYZ, _Q, _TRI = np.zeros(26), np.zeros(3, np.float32), np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32)
_PLANE = dict(normal=(0.0, 0.0, 1.0), anchor=(0.0, 0.0, 0.0))

# (HipCtx's method, Localizer's method, HIP symbol, Localizer symbol, arguments, keywords, the shape of the result when the call answers 0)
CASES = [
    ("map_seen_through", "map_seen_through", "flimo_map_seen_through", "flimo_loc_map_seen_through", (_X26, _XYZ), {}, ("bool:1", "int")),
    # (want_mask: HipCtx's alone before the two classes shared the method)
    ("map_seen_through", "map_seen_through", "flimo_map_seen_through", "flimo_loc_map_seen_through", (_X26, _XYZ), dict(want_mask=False),
     ("NoneType", "int")),
    ("map_carve", "map_carve", "flimo_map_carve", "flimo_loc_map_carve", (_X26, _XYZ), {}, "int"),
    ("map_carve", "map_carve", "flimo_map_carve", "flimo_loc_map_carve", (_X26, _XYZ), dict(box=(_XYZ, _XYZ)), "int"),
    ("map_outliers", "map_outliers", "flimo_map_outliers", "flimo_loc_map_outliers", (), {},
     {"mask": "bool:1", "mean_dist": "float64:1", "cnt": "int32:1", "stats": _OUTLIER_STATS}),
    ("map_remove_outliers", "map_remove_outliers", "flimo_map_remove_outliers", "flimo_loc_map_remove_outliers", (), {}, ("int", _OUTLIER_STATS)),
    ("map_fpfh", "map_fpfh", "flimo_map_fpfh", "flimo_loc_map_fpfh", (), {}, {"fpfh": "float32:2", "spfh": "uint8:2", "cnt": "int32:1"}),
    ("map_keypoints", "map_keypoints", "flimo_map_keypoints", "flimo_loc_map_keypoints", (), {},
     {"mask": "bool:1", "saliency": "float64:1", "cnt": "int32:1", "count": "int", "index": "int64:1"}),
    ("map_clusters", "map_clusters", "flimo_map_clusters", "flimo_loc_map_clusters", (), {},
     {"label": "int32:1", "size": "int32:1", "mask": "bool:1", "stats": _CLUSTER_STATS}),
    ("map_remove_clusters", "map_remove_clusters", "flimo_map_remove_clusters", "flimo_loc_map_remove_clusters", (), {}, ("int", _CLUSTER_STATS)),
    ("map_planes", "map_planes", "flimo_map_planes", "flimo_loc_map_planes", (_TRI,), {},
     {"status": "int32:1", "inliers": "int32:1", "sum_sq": "float64:1", "plane": "float64:2"}),
    ("map_plane_mask", "map_plane_mask", "flimo_map_plane_mask", "flimo_loc_map_plane_mask", (), _PLANE, ("bool:1", "int")),
    ("map_plane_mask", "map_plane_mask", "flimo_map_plane_mask", "flimo_loc_map_plane_mask", (), dict(_PLANE, want_mask=False), ("NoneType", "int")),
    ("map_remove_plane", "map_remove_plane", "flimo_map_remove_plane", "flimo_loc_map_remove_plane", (), _PLANE, "int"),
    ("map_voxels", "map_voxels", "flimo_map_voxels", "flimo_loc_map_voxels", (), {},
     {"ijk": "int32:2", "count": "int32:1", "centroid": "float64:2", "nv": "int", "stats": _VOXEL_STATS}),
    ("map_voxel_mask", "map_voxel_mask", "flimo_map_voxel_mask", "flimo_loc_map_voxel_mask", (), {},
     {"voxel": "int32:1", "mask": "bool:1", "stats": _VOXEL_STATS}),
    ("map_thin", "map_thin", "flimo_map_thin", "flimo_loc_map_thin", (), {}, ("int", _VOXEL_STATS)),
    ("map_regions", "map_regions", "flimo_map_regions", "flimo_loc_map_regions", (), {},
     {"label": "int32:1", "size": "int32:1", "mask": "bool:1", "stats": _REGION_STATS}),
    ("map_region_list", "map_region_list", "flimo_map_region_list", "flimo_loc_map_region_list", (), {},
     {"label": "int32:1", "count": "int32:1", "centroid": "float64:2", "cov": "float64:2", "nr": "int", "stats": _REGION_STATS}),
    ("map_remove_regions", "map_remove_regions", "flimo_map_remove_regions", "flimo_loc_map_remove_regions", (), {}, ("int", _REGION_STATS)),
    ("scan_fitness", "scan_fitness", "flimo_scan_fitness", "flimo_loc_scan_fitness", (np.zeros((2, 26)),), {}, ("int32:1", "float64:1")),
    ("scan_fitness", "scan_fitness", "flimo_scan_fitness", "flimo_loc_scan_fitness", (np.zeros((2, 26)),), dict(want_nn=True),
     ("int32:1", "float64:1", "float32:2", "int32:2")),
    ("scan_linearize", "scan_linearize", "flimo_scan_linearize", "flimo_loc_scan_linearize", (np.zeros((2, 26)), 5, 1.0), {},
     {"valid": "int32:1", "H": "float64:2", "g": "float64:2", "cost": "float64:1"}),
    ("scan_linearize", "scan_linearize", "flimo_scan_linearize", "flimo_loc_scan_linearize", (np.zeros((2, 26)), 5, 1.0), dict(want_rows=True),
     {"valid": "int32:1", "H": "float64:2", "g": "float64:2", "cost": "float64:1", "rows": "float64:3", "pair_cnt": "int32:2"}),
    ("corr_poses", "corr_poses", "flimo_corr_poses", "flimo_loc_corr_poses", (np.zeros((4, 3)), np.zeros((4, 3)), _TRI), dict(want=("pose", "pair_sqd")),
     {"status": "int32:1", "inliers": "int32:1", "sum_sqd": "float64:1", "pose": "float64:2", "pair_sqd": "float32:2"}),
    ("corr_graph", "corr_graph", "flimo_corr_graph", "flimo_loc_corr_graph", (np.zeros((4, 3)), np.zeros((4, 3))), dict(want=("adj",)),
     {"degree": "int32:1", "core": "int32:1", "adj": "uint64:2", "max_core": "int"}),
    ("desc_ref_set", "desc_ref_set", "flimo_desc_ref_set", "flimo_loc_desc_ref_set", (np.zeros((3, 8)),), {}, "NoneType"),
    ("desc_match", "desc_match", "flimo_desc_match", "flimo_loc_desc_match", (np.zeros((2, 8)),), {},
     {"idx": "int32:2", "dist": "float32:2", "cnt": "int32:1"}),
    ("knn_k", "map_knn", "flimo_knn_k", "flimo_loc_map_knn", (_Q, 3), {}, ("int32:2", "float32:2", "int32:1")),
    ("knn_k", "map_knn", "flimo_knn_k", "flimo_loc_map_knn", (_Q, 3), dict(want_xyz=True), ("int32:2", "float32:2", "int32:1", "float32:3")),
    ("radius_search", "map_radius_search", "flimo_radius_search", "flimo_loc_map_radius_search", (_Q, 1.0), {}, ("uint64:1", "int32:1", "float32:1")),
    ("radius_search", "map_radius_search", "flimo_radius_search", "flimo_loc_map_radius_search", (_Q, 1.0), dict(want_xyz=True),
     ("uint64:1", "int32:1", "float32:1", "float32:2")),
    ("normals", "map_normals", "flimo_map_normals", "flimo_loc_map_normals", (_Q, 5), {}, _NORMALS),
    # (the error of Localizer.map_normals_range named flimo_loc_map_normals before the two classes shared the method)
    ("normals_range", "map_normals_range", "flimo_map_normals_range", "flimo_loc_map_normals_range", (0, 2, 5), {}, _NORMALS),
]
_IDS = [f"{c[0]}{'-' + '-'.join(c[5]) if c[5] else ''}" for c in CASES]
_SIDES = [("hip", _hip_ctx, 0, 2), ("loc", _localizer, 1, 3)]


@pytest.mark.parametrize("side", _SIDES, ids=[s[0] for s in _SIDES])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_a_shared_method_calls_its_symbol_with_the_handle_first_and_shapes_the_result(case, side):
    _, make, method, symbol = side
    obj = make(0)
    out = getattr(obj, case[method])(*case[4], **case[5])
    calls = [(name, args) for name, args in obj._L.calls if name not in _SIZES]
    assert calls and {name for name, _ in calls} == {case[symbol]}
    assert all(args[0] is obj._h for _, args in calls)
    assert _shape(out) == case[6]
    if isinstance(out, dict):
        assert list(out) == list(case[6])      # (the order of the keys too)


@pytest.mark.parametrize("side", _SIDES, ids=[s[0] for s in _SIDES])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_a_shared_method_raises_its_class_error_on_a_non_zero_code(case, side):
    tag, make, method, symbol = side
    obj = make(-2)
    with pytest.raises(_lib.FlimoError) as err:
        getattr(obj, case[method])(*case[4], **case[5])
    assert str(err.value) == ("invalid argument: said the library" if tag == "hip" else f"{case[symbol]} failed (-2)")


def test_region_list_asks_again_with_room_for_every_region_and_only_then():
    """FLIMO_ERR_TOO_LARGE (-5) with *nr above the capacity: one more call with that capacity; with *nr within it: the error."""
    for make, symbol in ((_hip_ctx, "flimo_map_region_list"), (_localizer, "flimo_loc_map_region_list")):
        obj = make(0)
        caps = []

        def entry(h, cfg, cap, nr, *rest, _caps=caps):
            _caps.append(cap)
            nr._obj.value = 3000
            return -5 if cap < 3000 else 0
        setattr(obj._L, symbol, entry)
        out = obj.map_region_list()
        assert caps == [_lib.REGION_LIST_CAP, 3000] and out["nr"] == 3000 and out["label"].shape == (3000,) and out["cov"].shape == (3000, 6)
        obj = make(-5)
        with pytest.raises(_lib.FlimoError):
            obj.map_region_list()
        assert [name for name, _ in obj._L.calls].count(symbol) == 1


def test_unknown_outputs_are_refused_before_anything_is_called():
    for make in (_hip_ctx, _localizer):
        for method, args in (("map_outliers", ()), ("map_fpfh", ()), ("map_keypoints", ()), ("map_clusters", ()), ("map_planes", (_TRI,)),
                             ("map_voxels", ()), ("map_voxel_mask", ()), ("map_regions", ()), ("map_region_list", ()),
                             ("corr_poses", (_Q, _Q, _TRI)), ("corr_graph", (_Q, _Q))):
            obj = make(0)
            with pytest.raises(ValueError, match="unknown outputs"):
                getattr(obj, method)(*args, want=("no_such_output",))
            assert [name for name, _ in obj._L.calls if name not in _SIZES] == []
        with pytest.raises(ValueError, match="unknown outputs"):
            getattr(make(0), "normals" if make is _hip_ctx else "map_normals")(_Q, 5, want=("no_such_output",))


# ---- with the libraries loaded ----

def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(flimo_[A-Za-z0-9_]+)\s*\(", txt)))


def test_every_declared_function_has_argtypes(built):
    L, H = _lib.load_hip(), api.load_host()
    hip_decl = sorted(set(_declared("flimo_c.h") + _declared("flimo_dev.h")))
    host_decl = [name for name in _declared("flimo_localizer_c.h") if name not in hip_decl]
    assert len(hip_decl) >= 100 and len(host_decl) >= 60
    for lib, names in ((L, hip_decl), (H, host_decl)):
        for name in names:
            assert getattr(lib, name).argtypes is not None, name
    assert sorted(_lib.HIP_SYMBOLS) == hip_decl and sorted(api.HOST_SYMBOLS) == sorted(host_decl)
    assert L.flimo_version.argtypes == [] and L.flimo_version.restype is C.c_char_p


_RESULTS = {"int": C.c_int, "void": None, "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float, "const char*": C.c_char_p,
            "flimo_ctx*": C.c_void_p, "unsigned long long": C.c_ulonglong}


def _prototypes(header):
    """name -> (result as the header spells it, number of parameters) of every function ``header`` declares."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for m in re.finditer(r"(?m)^[ \t]*((?:const\s+)?(?:unsigned\s+long\s+long|[A-Za-z_0-9]+)\s*\*?)\s*(flimo_[A-Za-z0-9_]+)\s*\(", txt):
        depth, at, commas, body = 1, m.end(), 0, ""
        while depth:      # (to the matching parenthesis: a callback parameter has its own)
            c = txt[at]
            depth += (c == "(") - (c == ")")
            commas += c == "," and depth == 1
            body += c
            at += 1
        out[m.group(2)] = (re.sub(r"\s+", " ", m.group(1)).replace(" *", "*").strip(), 0 if body[:-1].strip() in ("", "void") else commas + 1)
    return out


def test_results_and_argument_counts_are_the_headers(built):
    L, H = _lib.load_hip(), api.load_host()
    seen = 0
    for lib, headers in ((L, ("flimo_c.h", "flimo_dev.h")), (H, ("flimo_localizer_c.h",))):
        for header in headers:
            for name, (result, count) in _prototypes(header).items():
                fn = getattr(lib, name)
                assert fn.restype is _RESULTS[result] and len(fn.argtypes) == count, (name, result, count)
                seen += 1
    assert seen == len(_lib.HIP_SYMBOLS) + len(api.HOST_SYMBOLS)


def test_both_symbols_of_a_paired_row_take_the_same_arguments(built):
    L, H = _lib.load_hip(), api.load_host()
    assert len(_abi.PAIRED) >= 27
    for hip, loc, args in _abi.PAIRED:
        assert list(getattr(L, hip).argtypes[1:]) == list(getattr(H, loc).argtypes[1:]) == list(args), hip
        assert getattr(L, hip).argtypes[0] is getattr(H, loc).argtypes[0] is C.c_void_p, hip
        assert hip in _lib.HIP_SYMBOLS and loc in api.HOST_SYMBOLS
    assert {case[2]: case[3] for case in CASES} == {hip: loc for hip, loc, _ in _abi.PAIRED}


def test_a_shared_method_is_one_function_on_both_classes():
    for case in CASES:
        assert getattr(_lib.HipCtx, case[0]) is getattr(api.Localizer, case[1]), case[0]
    for name in ("knn_k", "radius_search", "normals", "normals_range"):
        assert not hasattr(api.Localizer, name), name
    for name in ("map_knn", "map_radius_search", "map_normals", "map_normals_range"):
        assert not hasattr(_lib.HipCtx, name), name
    for name in ("_entry_chk", "_normals_chk", "_fitness_chk", "_linearize_chk", "_corr_chk"):
        assert not hasattr(api.Localizer, name), name
