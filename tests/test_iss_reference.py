"""CPU: the numpy restatement of ISS keypoints (tests/iss_reference.py) against an independent statement, the conditions
on the fixtures that the GPU tests (tests/test_iss_gpu.py) rest on, the C ABI of dh3d_iss_keypoints (declared, bound,
exported, every refusal a status code before anything touches the GPU) and the Python interface's refusals and signatures."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import iss_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dh3d_iss_keypoints_ws_bytes", "dh3d_iss_keypoints")
F = 256  # a non-null, 16-byte-aligned fake pointer: every check below fails before a launch
NATURAL = tuple(c for c in ref.CASE_IDS if c != "lattice")
SMALL = tuple(c for c in NATURAL if c.endswith("-small"))


def _independent(X, n, r_s):
    """Another statement of step 2: the members' two-pass centred covariance, then eigh."""
    X64 = X.astype(np.float64)
    lam = np.zeros((len(X), 3))
    for i in range(n):
        S = ref.membership(X, n, r_s, slice(i, i + 1))[0]
        pts = X64[:n][S]
        c = pts - pts.mean(0)
        lam[i] = np.linalg.eigh(c.T @ c / len(pts))[0][::-1]
    return lam


@pytest.mark.parametrize("case_id", NATURAL)
def test_restatement_against_an_independent_statement(case_id):
    X, n, r_s, r_n, res = ref.case(case_id)
    err = np.abs(res["lam"][:n] - _independent(X, n, r_s)[:n]).max() / r_s ** 2
    print(case_id, "max |lam - lam'| / r_s^2 = %.3g" % err)
    assert err <= 1e-13
    assert (res["num_nbr"][:n] >= 1).all() and not res["num_nbr"][n:].any() and not res["saliency"][n:].any()
    assert (np.diff(res["lam"], axis=1) <= 0).all()


@pytest.mark.parametrize("case_id", NATURAL)
def test_margins_and_shells_of_the_fixtures(case_id):
    X, n, r_s, r_n, res = ref.case(case_id)
    low = res["margin"][:n].min()
    print(case_id, "smallest decision margin %.3g" % low)
    assert low >= 4e-12                                       # the GPU's saliency test leaves no row out
    assert ref.shell_pairs(X, n, r_s) == 0 and ref.shell_pairs(X, n, r_n) == 0


@pytest.mark.parametrize("case_id", SMALL)
def test_keypoints_and_ties_of_the_fixtures(case_id):
    X, n, r_s, r_n, res = ref.case(case_id)
    key, tie = ref.keypoint_mask(X, n, r_n, res["saliency"], res["num_nbr"][:, 1])
    print(case_id, "keypoints", int(key.sum()), "decided by the tie rule", int(tie.sum()))
    assert key.sum() >= 20
    if not case_id.startswith("dso_9000_cut"):
        assert tie.sum() >= 10                                # the scene and the demo clouds
    ids, count = ref.select(key, res["saliency"], 16)
    assert count == 16 and (np.diff(res["saliency"][ids].astype(np.float64)) <= 0).all()


def test_grid_paths_of_the_fixtures():
    """Which walk the kernel takes where: the cube is not crowded and its boxes hold at most 512 cells at 5 m and more at
    12 m (the group walk); the demo clouds are crowded, and the kernel stays on their cells."""
    for case_id, crowded, wide in (("cube-5-4", 0, False), ("cube-wide", 0, True), ("local_642-small", 1, False),
                                   ("global_c-small", 1, False), ("dso_9000-small", 1, False), ("dso_9000_cut-small", 1, False),
                                   ("global_c-wide", 1, True), ("scene0-wide", None, True)):
        X, n, r_s, r_n, _ = ref.case(case_id)
        flag, cells = ref.grid_facts(X, n, max(r_s, r_n))
        print(case_id, "crowded", flag, "box cells", cells.min(), "..", cells.max())
        assert crowded is None or flag == crowded, case_id
        assert (cells.max() > 512) == wide, case_id
        if not wide:
            assert cells.max() <= 512
    X, n, r_s, r_n, _ = ref.case("cube-wide")
    cells = ref.grid_facts(X, n, r_s)[1]
    assert (cells <= 512).any() and (cells > 512).any()       # both walks in one launch


def test_cube_wide_runs_both_walks_in_one_wave():
    """csrc/cell_walk.h's walk has two halves, a lane's cells and the wave-uniform group loop; the case that can go wrong is
    a wave that runs both, with the suppression's early exits.  The lanes of a wave are 64 consecutive sorted positions: at
    both radii of `cube-wide` (the moments kernel walks at max(r_s, r_n), the suppression at r_n) at least half of the 32
    waves hold a lane at or below the 512-cell limit and a lane above it, so the bit-equal count and selection tests on
    this fixture run the mixed wave."""
    X, n, r_s, r_n, _ = ref.case("cube-wide")
    assert n == len(X) == 2048
    order = ref.sr.restate(ref.packed(X, n))["order"]         # sorted position -> point
    for r in (max(r_s, r_n), r_n):
        wide = (ref.grid_facts(X, n, r)[1][order] > 512).reshape(32, 64)
        mixed = int((wide.any(1) & ~wide.all(1)).sum())
        print("r = %.1f: waves with both walks %d of 32, points above the limit %.0f %%" % (r, mixed, 100.0 * wide.mean()))
        assert mixed >= 16


def test_lattice_has_pairs_on_the_shell():
    X, n, r_s, r_n, res = ref.case("lattice")
    assert ref.shell_pairs(X, n, r_s) > 1000 and ref.shell_pairs(X, n, r_n) > 1000
    inner = res["num_nbr"][np.all((X > 1.4) & (X < 4.1), axis=1)]
    assert (inner == inner[0]).all() and inner[0, 0] == 93 and inner[0, 1] == 27   # strict: the shells at 1.5 and 1.0 stay out


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                     # an addition only
    assert _lib._RESTYPES["dh3d_iss_keypoints_ws_bytes"] is ctypes.c_size_t
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "iss.o" in exact                                                           # built without contraction
    said = header[header.index("ISS keypoints (csrc/iss.hip)"):header.index("size_t dh3d_iss_keypoints_ws_bytes(")]
    for word in ("INFERRED", "d2 < r_s * r_s", "NOT the float32 d", "lowest index", "gamma_21 * l1", "min_neighbors",
                 "graph-capturable", "Every element of every output is written", "saliency_in"):
        assert word in said, word


def _call(lib, xyz=F, stride=3, count=F, radii=F, sal_in=None, P=2, N=1000, g21=0.975, g32=0.975, min_nb=5, M=100, sal=F, nbr=F,
          lam=None, ids=F, kpc=F, ws=F, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return lib.dh3d_iss_keypoints(xyz, stride, count, radii, sal_in, P, N, g21, g32, min_nb, M, sal, nbr, lam, ids, kpc, ws,
                                  ws_bytes, None)


def test_refusals():
    from dh3d_amd import _lib
    lib = _lib.lib()
    nan = float("nan")
    for kw in (dict(xyz=None), dict(radii=None), dict(sal=None), dict(nbr=None), dict(ids=None), dict(kpc=None), dict(ws=None),
               dict(ws=264), dict(stride=2), dict(P=0), dict(P=-1), dict(N=0), dict(N=-5), dict(M=0), dict(M=-1), dict(min_nb=0),
               dict(g21=0.0), dict(g21=1.5), dict(g21=nan), dict(g32=0.0), dict(g32=-0.1), dict(g32=nan),
               dict(ws_bytes=lib.dh3d_iss_keypoints_ws_bytes(2, 1000, 100) - 1), dict(ws_bytes=0)):
        assert _call(lib, **kw) == 1, kw
    for kw in (dict(N=16385), dict(P=65536), dict(M=4097)):
        assert _call(lib, **kw) == 2, kw


def test_ws_bytes_rows():
    from dh3d_amd import _lib
    ws = _lib.lib().dh3d_iss_keypoints_ws_bytes
    for P, N, M in ((1, 1, 1), (2, 1000, 100), (6, 2048, 4096), (64, 8192, 4096), (65535, 64, 1), (1, 16384, 4096)):
        groups = (N + 63) // 64
        # the sort's records, group boxes and cell table, the packed copy, the sorted saliencies, the keys: 16-byte segments
        want = sum((b + 15) & ~15 for b in (16 * P * N, 32 * P * groups, 4 * 4112 * P, 12 * P * N, 4 * P * N, 8 * P * N))
        assert ws(P, N, M) == want, (P, N, M)
    for P, N, M in ((0, 100, 10), (-1, 100, 10), (1, 0, 10), (1, 16385, 10), (65536, 100, 10), (1, 100, 0), (1, 100, 4097)):
        assert ws(P, N, M) == 0, (P, N, M)


def test_python_interface():
    from dh3d_amd import registration as reg
    a = torch.zeros(2, 50, 3)
    with pytest.raises(ValueError, match="GPU"):
        reg.iss_keypoints(a)                                      # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        reg.cloud_resolution(a)
    with pytest.raises(ValueError, match="GPU"):
        reg.register_fpfh(a, a, keypoints={"method": "iss"})
    with pytest.raises(ValueError, match="method"):
        reg._fpfh_keypoints(a, None, {"method": "nope"}, None, "anchor")
    with pytest.raises(ValueError, match="method"):
        reg._fpfh_keypoints(a, None, {"salient_radius": 2.0}, None, "anchor")
    sig = inspect.signature(reg.iss_keypoints)
    assert list(sig.parameters) == ["points", "num_valid", "salient_radius", "non_max_radius", "gamma_21", "gamma_32",
                                    "min_neighbors", "max_keypoints", "saliency", "eigenvalues"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["num_valid"], d["salient_radius"], d["non_max_radius"], d["gamma_21"], d["gamma_32"], d["min_neighbors"],
            d["max_keypoints"], d["saliency"], d["eigenvalues"]) == (None, None, None, 0.975, 0.975, 5, 4096, None, False)
    sig = inspect.signature(reg.cloud_resolution)
    assert list(sig.parameters) == ["points", "num_valid"] and sig.parameters["num_valid"].default is None
    sig = inspect.signature(reg.register_fpfh)                    # unchanged: the detector is a new VALUE of `keypoints`
    assert list(sig.parameters) == ["anchor_points", "positive_points", "num_valid", "keypoints", "keypoint_ids", "k",
                                    "max_dist", "refine", "ransac_kw"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["num_valid"], d["keypoints"], d["keypoint_ids"], d["k"], d["max_dist"], d["refine"]) == (None, None, None, 32, None, None)
    assert reg.ISS_MAX_POINTS == 16384


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the checks of the Python layer that come before any launch."""
    @property
    def is_cuda(self):
        return True


def test_python_refusals_before_any_launch():
    from dh3d_amd import registration as reg
    big = torch.zeros(1, 16385, 3).as_subclass(_FakeCuda)
    with pytest.raises(ValueError, match="16384"):
        reg.iss_keypoints(big, salient_radius=1.0, non_max_radius=1.0)
    x = torch.zeros(1, 64, 3).as_subclass(_FakeCuda)
    with pytest.raises(ValueError, match="max_keypoints"):
        reg.iss_keypoints(x, salient_radius=1.0, non_max_radius=1.0, max_keypoints=4097)
    with pytest.raises(ValueError, match="max_keypoints"):
        reg.iss_keypoints(x, salient_radius=1.0, non_max_radius=1.0, max_keypoints=0)
    for kw in (dict(gamma_21=0.0), dict(gamma_21=1.01), dict(gamma_32=float("nan")), dict(gamma_32=-1.0)):
        with pytest.raises(ValueError, match="gamma"):
            reg.iss_keypoints(x, salient_radius=1.0, non_max_radius=1.0, **kw)
    with pytest.raises(ValueError, match="min_neighbors"):
        reg.iss_keypoints(x, salient_radius=1.0, non_max_radius=1.0, min_neighbors=0)
