"""CPU: dh3d_gnc_rigid (include/dh3d_hip.h, csrc/registration.hip) is declared, bound and exported; every refusal is a
status code before anything touches the GPU, an invalid argument ahead of an unsupported shape; the Python interface
refuses what the kernel does not take and keeps the estimators' keywords apart."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 256  # a non-null fake pointer: every check below fails before a launch


def test_symbol_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+dh3d_gnc_rigid\s*\(", header)
    assert "dh3d_gnc_rigid" in _lib.EXPORTED_SYMBOLS and hasattr(handle, "dh3d_gnc_rigid")
    assert header.index("int dh3d_gnc_rigid(") > header.index("int dh3d_ransac_rigid(")  # beside the estimator it joins
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                        # an addition only
    assert re.search(r"#define\s+DH3D_ABI_VERSION\s+4\b", header)
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "registration.o" in exact                                                     # built without contraction
    said = header[header.index("Graduated non-convexity"):header.index("int dh3d_gnc_rigid(")]
    for word in ("Geman-McClure", "n < 3", "D2", "d2 = threshold * threshold", "mu == d2", "at > settle", "k >= max_iterations",
                 "(mu / (|r_j|^2 + mu))^2", "mu / division", "weighted_fit", "cx = (sum w X) / W", "(xc - R yc) + t",
                 "never stored", "not a guarantee", "graph-capturable", "every element written"):
        assert word in said, word
    assert len(_lib._SIGNATURES["dh3d_gnc_rigid"]) == 21


def _gnc(lib, ax=F, bx=F, m=F, ac=F, P=2, Ma=512, Mb=512, thr=1.0, division=1.4, settle=8, iters=64, sa=132, sb=132, **out):
    o = dict(Rt=F, weights=F, valid=F, inliers=F, num_inliers=F, num_corr=F, iterations=F)
    o.update(out)
    return lib.dh3d_gnc_rigid(ax, sa, bx, sb, m, ac, P, Ma, Mb, thr, division, settle, iters, o["Rt"], o["weights"], o["valid"],
                              o["inliers"], o["num_inliers"], o["num_corr"], o["iterations"], None)


INVALID = (dict(ax=None), dict(bx=None), dict(m=None), dict(ac=None), dict(Rt=None), dict(weights=None), dict(valid=None),
           dict(inliers=None), dict(num_inliers=None), dict(num_corr=None), dict(iterations=None),
           dict(P=0), dict(P=-1), dict(Ma=0), dict(Ma=-5), dict(Mb=0), dict(Mb=-5), dict(sa=2), dict(sb=2), dict(sa=0),
           dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")), dict(division=1.0), dict(division=0.5),
           dict(division=float("nan")), dict(settle=-1), dict(iters=0), dict(iters=-3), dict(iters=1025))
UNSUPPORTED = (dict(Ma=4097), dict(Mb=4097), dict(P=65536))


def test_status_codes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for kw in INVALID:
        assert _gnc(lib, **kw) == 1, kw
    for kw in UNSUPPORTED:
        assert _gnc(lib, **kw) == 2, kw
    for bad in INVALID:       # an invalid argument is reported ahead of an unsupported shape
        for big in UNSUPPORTED:
            if not set(bad) & set(big):
                assert _gnc(lib, **bad, **big) == 1, (bad, big)


def test_python_interface():
    from dh3d_amd import registration as reg
    cpu = torch.zeros(1, 8, 132)
    cnt = torch.zeros(1, dtype=torch.int32)
    ids = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        reg.gnc_rigid(cpu, cpu, ids, cnt)                          # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        reg.register(cpu, cnt, cpu, cnt, estimator="gnc")
    sig = inspect.signature(reg.gnc_rigid)
    assert list(sig.parameters) == ["anchor_xyz", "positive_xyz", "match", "anchor_count", "threshold", "division", "settle",
                                    "max_iterations"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["threshold"], d["division"], d["settle"], d["max_iterations"]) == (1.0, 1.4, 8, 64)
    assert d["threshold"] == inspect.signature(reg.ransac_rigid).parameters["threshold"].default
    # the estimator is chosen, and its keywords checked, before a tensor is looked at
    fit = lambda **kw: reg._match_and_fit(cpu, cnt, cpu, cnt, cpu, cpu, None, kw)
    with pytest.raises(ValueError, match="estimator must be"):
        fit(estimator="lmeds")
    with pytest.raises(ValueError, match="estimator must be"):
        fit(estimator=None)
    with pytest.raises(ValueError, match='estimator="gnc".*seed'):
        fit(estimator="gnc", seed=1)
    with pytest.raises(ValueError, match='estimator="gnc".*confidence'):
        fit(estimator="gnc", confidence=0.9)
    with pytest.raises(ValueError, match='estimator="ransac".*division'):
        fit(estimator="ransac", division=2.0)
    with pytest.raises(ValueError, match='estimator="ransac".*settle'):
        fit(settle=3)                                              # the default estimator is RANSAC
    # ... and register / register_fpfh / register_clouds refuse it before they launch anything (CPU tensors never get looked at)
    with pytest.raises(ValueError, match="estimator must be"):
        reg.register(cpu, cnt, cpu, cnt, estimator="lmeds")
    with pytest.raises(ValueError, match='estimator="gnc".*seed'):
        reg.register(cpu, cnt, cpu, cnt, estimator="gnc", seed=1)
    with pytest.raises(ValueError, match='estimator="gnc".*seed'):
        reg.register_fpfh(cpu, cpu, estimator="gnc", seed=1, match={"ratio": 0.9})
    with pytest.raises(ValueError, match='estimator="ransac".*division'):
        reg.register_fpfh(cpu, cpu, division=2.0)

    class _Model(object):
        class config(object):
            detection = True

        def forward(self, *a, **k):
            raise AssertionError("the estimator is checked before the forwards run")
    with pytest.raises(ValueError, match='estimator="gnc".*max_trials'):
        reg.register_clouds(_Model(), cpu, cpu, estimator="gnc", max_trials=5, desc_dim=128)
    assert reg._estimator({}) == (reg.ransac_rigid, {})
    assert reg._estimator(dict(estimator="ransac", seed=3)) == (reg.ransac_rigid, dict(seed=3))
    assert reg._estimator(dict(estimator="gnc", threshold=0.5, settle=2)) == (reg.gnc_rigid, dict(threshold=0.5, settle=2))
    assert "trials" in reg.gnc_rigid.__doc__ and "not a guarantee" in reg.gnc_rigid.__doc__
