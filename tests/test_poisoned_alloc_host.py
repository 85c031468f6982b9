"""Host: the poisoned-allocation harness (tests/poisoned_alloc.py) does what tests/test_unwritten_memory_gpu.py relies
on, checked on CPU tensors (the device check lifted by `_cpu_too`, which only this file uses), and dh3d_amd obtains
uninitialised memory by no route the harness does not wrap."""
import ast
import math
import os

import pytest
import torch

import poisoned_alloc as PA

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dh3d_amd")


def _originals():
    return [getattr(owner, name) for owner, name in PA.ENTRY_POINTS]


def test_entry_points_wrapped_and_restored():
    from dh3d_amd import registration
    before = _originals()
    registration._ICP_WS["probe"] = torch.zeros(1)
    cached = list(registration._ICP_WS)   # ("probe" behind whatever earlier tests of the same process left there)
    try:
        with PA.poisoned("pos"):
            inside = _originals()
            assert all(a is not b for a, b in zip(inside, before))
            assert all(a.__wrapped__ is b for a, b in zip(inside, before))
            assert not registration._ICP_WS and not registration._ISS_WS     # cached workspaces are allocated again
            registration._ISS_WS["inside"] = torch.zeros(1)
        assert all(a is b for a, b in zip(_originals(), before))
        assert list(registration._ICP_WS) == cached and "inside" not in registration._ISS_WS
        with pytest.raises(KeyError):
            with PA.poisoned("nan"):
                raise KeyError("from inside")
        assert all(a is b for a, b in zip(_originals(), before))
        assert list(registration._ICP_WS) == cached
        with pytest.raises(ValueError):
            with PA.poisoned("big"):
                pass
        with PA.poisoned("neg"):
            with pytest.raises(RuntimeError):
                with PA.poisoned("pos"):
                    pass
        assert all(a is b for a, b in zip(_originals(), before))
        with PA.poisoned(None):                                              # the plain run replaces nothing
            assert all(a is b for a, b in zip(_originals(), before))
    finally:
        registration._ICP_WS.pop("probe", None)


@pytest.mark.parametrize("kind,f,i,u", [("nan", math.nan, 0, 0x00), ("pos", 1e30, 1, 0xFF), ("neg", -1e30, 0, 0x00)])
def test_fill_values_by_dtype(kind, f, i, u):
    def same(t, v):
        if isinstance(v, float) and math.isnan(v):
            return bool(torch.isnan(t).all())
        return bool((t == torch.tensor(v, dtype=t.dtype)).all())

    base = torch.zeros((2, 3), dtype=torch.float32)
    with PA.poisoned(kind, _cpu_too=True):
        for dt in (torch.float32, torch.float64, torch.bfloat16):
            assert same(torch.empty((3, 5), dtype=dt), f), dt
        half = f if math.isnan(f) else math.copysign(65504.0, f)             # float16 cannot hold 1e30
        assert same(torch.empty((3, 5), dtype=torch.float16), half)
        for dt in (torch.int32, torch.int64, torch.int16):
            assert same(torch.empty((3, 5), dtype=dt), i), dt
        assert same(torch.empty((7,), dtype=torch.uint8), u)
        assert same(torch.empty((7,), dtype=torch.bool), bool(i))
        assert same(torch.empty(4, 2), f)                                    # sizes as positional arguments
        assert same(torch.empty_like(base), f) and same(torch.empty_like(base, dtype=torch.int32), i)
        assert same(base.new_empty((4,)), f) and same(base.new_empty((4,), dtype=torch.uint8), u)
        assert torch.empty((0, 3)).numel() == 0
    # without the flag CPU tensors are left alone
    assert bool((PA._poison(torch.zeros(64), kind, False) == 0).all())
    assert same(PA._poison(torch.zeros(64), kind, True), f)


def test_zero_element_set_view_is_untouched():
    """pm.ZeroArena.take: torch.empty((0,)).set_(storage, offset, shape) must hand out the arena's zeros."""
    buf = torch.zeros((1024,), dtype=torch.uint8)
    with PA.poisoned("pos", _cpu_too=True):
        v = torch.empty((0,), dtype=torch.float32).set_(buf.untyped_storage(), 4, (3, 5))
        assert v.shape == (3, 5) and bool((v == 0).all())
    assert bool((buf == 0).all())


def test_zero_arena_views_stay_zero_on_the_cpu():
    from dh3d_amd import pm
    with PA.poisoned("pos", _cpu_too=True):
        a = pm.ZeroArena(fixed_bytes=4096, device="cpu")
        assert bool((a.buf == 0xFF).all())
        a.begin(torch.device("cpu"))
        v = a.take((3, 7), torch.float64, torch.device("cpu"))
        assert bool((v == 0).all())


def test_nn_and_optimizer_work_inside():
    torch.manual_seed(0)
    with PA.poisoned("nan", _cpu_too=True):
        lin = torch.nn.Linear(5, 3)
        assert all(bool(torch.isfinite(p).all()) for p in lin.parameters())
        opt = torch.optim.Adam(lin.parameters(), lr=1e-2)
        w0 = lin.weight.detach().clone()
        loss = lin(torch.ones(4, 5)).square().sum()
        loss.backward()
        opt.step()
        assert all(bool(torch.isfinite(p).all()) for p in lin.parameters())
        assert not torch.equal(w0, lin.weight.detach())
        assert torch.empty((2,), requires_grad=True).requires_grad          # a leaf that requires grad can be filled


# ------------------------------------------------------------------------------------------------ completeness
WRAPPED = {"empty", "empty_like", "new_empty"}
# names that hand out uninitialised memory and are NOT wrapped
UNWRAPPED = {"empty_strided", "new_empty_strided", "empty_permuted", "empty_quantized", "_empty_affine_quantized",
             "resize_", "resize_as_", "resize"}
LEGACY = {"Tensor", "FloatTensor", "DoubleTensor", "HalfTensor", "BFloat16Tensor", "IntTensor", "LongTensor",
          "ShortTensor", "CharTensor", "ByteTensor", "BoolTensor", "Storage", "UntypedStorage", "TypedStorage"}


def unwrapped_routes(source, filename="<src>"):
    """(line, what) for every way `source` obtains uninitialised memory that poisoned() does not see."""
    tree = ast.parse(source, filename)
    called = {id(n.func) for n in ast.walk(tree) if isinstance(n, ast.Call)}
    torch_names = {"torch"}
    for n in ast.walk(tree):
        if isinstance(n, ast.Import):
            torch_names |= {a.asname or a.name for a in n.names if a.name == "torch"}
    found = []

    def is_torch(node):  # torch, torch.cuda
        return (isinstance(node, ast.Name) and node.id in torch_names) or (
            isinstance(node, ast.Attribute) and node.attr == "cuda" and is_torch(node.value))

    for n in ast.walk(tree):
        if isinstance(n, ast.ImportFrom) and n.module and n.module.split(".")[0] == "torch":
            for a in n.names:
                if a.name in WRAPPED | UNWRAPPED | LEGACY or a.name == "*":
                    found.append((n.lineno, "from %s import %s" % (n.module, a.name)))
        elif isinstance(n, ast.Attribute):
            if n.attr in UNWRAPPED:
                found.append((n.lineno, "." + n.attr))
            elif n.attr in LEGACY and is_torch(n.value) and id(n) in called:
                found.append((n.lineno, "legacy constructor torch.%s(...)" % n.attr))
            elif n.attr == "new" and id(n) in called:
                found.append((n.lineno, "legacy constructor .new(...)"))
            elif n.attr in WRAPPED and id(n) not in called:
                found.append((n.lineno, ".%s bound to another name or passed on" % n.attr))
        elif isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "getattr" and len(n.args) >= 2 \
                and isinstance(n.args[1], ast.Constant) and n.args[1].value in WRAPPED | UNWRAPPED | LEGACY:
            found.append((n.lineno, "getattr(..., %r)" % n.args[1].value))
        elif isinstance(n, ast.Name) and n.id in WRAPPED | UNWRAPPED and isinstance(n.ctx, ast.Load):
            found.append((n.lineno, "bare name %s" % n.id))
    return found


def test_completeness_check_sees_every_route():
    bad = {
        "import torch\nx = torch.empty_strided((2,), (1,))": "empty_strided",
        "def f(t):\n    t.resize_(4)": "resize_",
        "import torch\nx = torch.FloatTensor(3)": "FloatTensor",
        "import torch\nx = torch.cuda.FloatTensor(3)": "FloatTensor",
        "import torch\nx = torch.Tensor(3)": "Tensor",
        "def f(t):\n    return t.new(3)": ".new(",
        "from torch import empty\nx = empty(3)": "import empty",
        "import torch\nalloc = torch.empty\nx = alloc(3)": "bound",
        "import torch\ndef f(n, alloc=torch.empty_like):\n    return alloc(n)": "bound",
        "import torch as th\nx = getattr(th, 'empty')(3)": "getattr",
        "import torch\nx = map(torch.Tensor.new_empty, [])": "bound",
    }
    for src, what in bad.items():
        got = unwrapped_routes(src)
        assert got and any(what in w for _, w in got), (src, got)
    good = ("import torch\nx = torch.empty((3,), dtype=torch.int32)\ny = torch.empty_like(x)\nz = x.new_empty((2,))\n"
            "w = torch.empty((0,)).set_(x.untyped_storage(), 0, (3,))\nisinstance(x, torch.Tensor)\n")
    assert unwrapped_routes(good) == []


def test_dh3d_amd_allocates_only_through_wrapped_entry_points():
    files = sorted(os.path.join(d, f) for d, _, fs in os.walk(PKG) for f in fs if f.endswith(".py"))
    assert len(files) >= 20, files
    found, sites = [], 0
    for path in files:
        with open(path) as fh:
            src = fh.read()
        found += [(os.path.relpath(path, PKG), line, what) for line, what in unwrapped_routes(src, path)]
        sites += sum(isinstance(n, ast.Attribute) and n.attr in WRAPPED for n in ast.walk(ast.parse(src)))
    assert not found, "uninitialised memory by a route tests/poisoned_alloc.py does not wrap: %s" % (found,)
    assert sites >= 200, sites     # the wrapped sites are there to be poisoned (224 when this test was written)
