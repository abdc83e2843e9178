"""The poisoning helper of tests/poison.py, checked without a GPU: the fill is exact for every dtype the package allocates, the
initialised allocators stay as they are, no module of the package that calls an uninitialised allocator is missing from the helper's
list, and the comparator reports a read-before-write / unwritten-element function as differing (and a correct one as equal)."""
import ast
import os
import types

import pytest
import torch

import sol_amd
import poison

PKG = os.path.dirname(os.path.abspath(sol_amd.__file__))
# torch's allocators that return memory without writing it (factory functions and Tensor methods)
ALLOCATORS = {"empty", "empty_like", "empty_strided", "empty_permuted", "new_empty", "new_empty_strided", "empty_quantized", "resize_",
              "FloatTensor", "IntTensor", "LongTensor", "DoubleTensor", "HalfTensor", "ByteTensor"}


def _package_modules():
    """(dotted module name, path) of every module of the package: *.py of the package directory and of its sub-packages (directories
    with an __init__.py)"""
    out = []
    for root, dirs, files in os.walk(PKG):
        dirs[:] = sorted(d for d in dirs if os.path.isfile(os.path.join(root, d, "__init__.py")))
        rel = os.path.relpath(root, PKG)
        prefix = "" if rel == "." else rel.replace(os.sep, ".") + "."
        out += [(prefix + f[:-3], os.path.join(root, f)) for f in sorted(files) if f.endswith(".py") and f != "__init__.py"]
        if rel != ".":
            out.append((rel.replace(os.sep, "."), os.path.join(root, "__init__.py")))
    out.append(("", os.path.join(PKG, "__init__.py")))
    return out


def _allocator_calls(path):
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    found = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call):
            fn = node.func
            name = fn.attr if isinstance(fn, ast.Attribute) else fn.id if isinstance(fn, ast.Name) else None
            if name in ALLOCATORS:
                found.append((name, node.lineno))
    return found


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.int16, torch.float16])
@pytest.mark.parametrize("shape", [(7,), (3, 5), (2, 3, 5, 4), (1,), ()])
def test_fill_writes_the_exact_pattern_for_every_dtype(pattern, dtype, shape):
    proxy = poison.TorchProxy(pattern)
    t = proxy.empty(*shape, dtype=dtype) if shape else proxy.empty((), dtype=dtype)
    assert t.dtype == dtype and tuple(t.shape) == shape
    raw = bytes(t.contiguous().reshape(-1).view(torch.uint8).tolist())
    want = (pattern.to_bytes(4, "little") * (len(raw) // 4 + 1))[:len(raw)]
    assert raw == want
    u = proxy.empty_like(torch.zeros(shape, dtype=dtype))
    assert u.dtype == dtype and bytes(u.contiguous().reshape(-1).view(torch.uint8).tolist()) == want


def test_fill_values_are_what_the_pattern_table_says():
    f = lambda p, dt: poison.TorchProxy(p).empty(4, dtype=dt)
    assert bool(torch.isnan(f(poison.ALL_ONES, torch.float32)).all())
    assert f(poison.ALL_ONES, torch.int32).tolist() == [-1] * 4 and f(poison.ALL_ONES, torch.int64).tolist() == [-1] * 4
    assert f(poison.FLT_MAX, torch.float32).tolist() == [float(torch.finfo(torch.float32).max)] * 4
    one = f(poison.ONE, torch.float32)
    assert bool((one > 0).all()) and bool((one < torch.finfo(torch.float32).tiny).all()) and f(poison.ONE, torch.int32).tolist() == [1] * 4
    assert f(poison.ZERO, torch.float64).tolist() == [0.0] * 4


def test_fill_covers_a_memory_format_and_an_empty_tensor():
    proxy = poison.TorchProxy(poison.FLT_MAX)
    src = torch.zeros(2, 3, 4, 5, dtype=torch.float32).to(memory_format=torch.channels_last)
    t = proxy.empty_like(src)
    assert t.stride() == src.stride() and bool((t == torch.finfo(torch.float32).max).all())
    t = proxy.empty_like(src.permute(0, 2, 3, 1), memory_format=torch.contiguous_format)
    assert t.is_contiguous() and bool((t == torch.finfo(torch.float32).max).all())
    assert proxy.empty(0, dtype=torch.float32).numel() == 0


def test_everything_else_is_the_real_torch():
    proxy = poison.TorchProxy(poison.ALL_ONES)
    for name in ("zeros", "zeros_like", "full", "ones", "tensor", "Tensor", "float32", "cuda", "autograd", "no_grad", "from_numpy"):
        assert getattr(proxy, name) is getattr(torch, name)
    assert proxy.zeros(5).tolist() == [0.0] * 5 and proxy.ones(2, dtype=torch.int32).tolist() == [1, 1] and proxy.full((2,), 3.0).tolist() == [3.0, 3.0]
    assert isinstance(proxy.empty(2), proxy.Tensor)


def test_the_helper_lists_every_module_that_calls_an_uninitialised_allocator():
    """A new module (or a new allocator) cannot be forgotten: every module of the package whose source calls an uninitialised
    allocator is in poison.MODULES, every name it calls is one the stand-in replaces, and MODULES names no module that has none."""
    calling = {}
    for name, path in _package_modules():
        calls = _allocator_calls(path)
        if calls:
            calling[name] = calls
    assert calling, "the walk found no allocator call at all: it is looking in the wrong place (%s)" % PKG
    missing = sorted(set(calling) - set(poison.MODULES))
    assert not missing, "modules that call torch.empty & co. but are not poisoned: %s" % {m: calling[m] for m in missing}
    stale = sorted(set(poison.MODULES) - set(calling))
    assert not stale, "poison.MODULES names modules without such a call: %s" % stale
    other = sorted({(m, n, line) for m, c in calling.items() for n, line in c if n not in poison.UNINITIALISED})
    assert not other, "uninitialised allocators the stand-in does not replace: %s" % other
    for mod in poison.modules():
        assert mod.torch is torch, "%s does not reach torch through a module global named `torch`" % mod.__name__


def test_the_scripts_directory_is_no_package():
    """poison.MODULES leaves the command-line programs out because they are no modules of the package; if that changes they must be
    covered like the rest."""
    assert not os.path.exists(os.path.join(PKG, "scripts", "__init__.py"))


def test_poisoned_installs_and_removes_the_stand_in(monkeypatch):
    mods = poison.modules()
    with poison.pattern(monkeypatch, poison.FLT_MAX) as proxy:
        assert all(m.torch is proxy for m in mods)
        assert sol_amd._lib.torch.empty(3, dtype=torch.float32).tolist() == [float(torch.finfo(torch.float32).max)] * 3
        import torch as real
        assert real is torch and not isinstance(real, poison.TorchProxy)
    assert all(m.torch is torch for m in mods)


# ---- the comparator has teeth ------------------------------------------------------------------------------------------------------
def _toy_module():
    """A module-like object with functions that allocate through the module global `torch`, as the package's do"""
    mod = types.ModuleType("toy")
    mod.torch = torch
    src = '''
def correct(x):
    out = torch.empty_like(x)
    out.copy_(x * 2.0)
    return out, {"iterations": torch.full((2,), 7, dtype=torch.int32)}

def leaves_one_element(x):
    out = torch.empty_like(x)
    out.reshape(-1)[:-1].copy_(x.reshape(-1)[:-1] * 2.0)          # the last element is never written
    return out, {"iterations": torch.full((2,), 7, dtype=torch.int32)}

def reads_scratch_first(x):
    ws = torch.empty(x.numel(), dtype=torch.float32)
    ws[1:] = 0.0                                                  # the clear misses word 0
    ws += x.reshape(-1)                                           # ... which the accumulation then reads
    return ws.reshape(x.shape).clone()

def stale_flag(x):
    done = torch.empty(1, dtype=torch.int32)
    return x * 2.0 if int(done) == 0 else x                       # a `done` word taken from the last call
'''
    exec(compile(src, "toy", "exec"), mod.__dict__)
    return mod


def _differs(monkeypatch, mod, fn):
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4) + 1.0
    runs = []
    for p in poison.PATTERNS:
        with monkeypatch.context() as m:
            m.setattr(mod, "torch", poison.TorchProxy(p))
            runs.append(poison.snapshot(fn(x)))
    return [poison.first_difference(r, runs[0], fn.__name__) for r in runs[1:]], runs


def test_comparator_reports_an_unwritten_element_and_a_read_before_write(monkeypatch):
    mod = _toy_module()
    diffs, _ = _differs(monkeypatch, mod, mod.correct)
    assert diffs == [None, None, None]
    diffs, runs = _differs(monkeypatch, mod, mod.leaves_one_element)
    assert all(d is not None for d in diffs), diffs
    assert "word 11 of 12" in diffs[0] and "leaves_one_element[0]" in diffs[0], diffs[0]
    assert poison.leaked_pattern(runs[1], runs[0]) is not None and poison.leaked_pattern(runs[2], runs[0]) is not None
    diffs, _ = _differs(monkeypatch, mod, mod.reads_scratch_first)
    # (the denormal of pattern 1 is absorbed by an fp32 sum with 1.0: that pattern is there for flags and integer words)
    assert all(d is not None and "word 0 of 12" in d for d in diffs[:2]) and diffs[2] is None, diffs
    diffs, _ = _differs(monkeypatch, mod, mod.stale_flag)
    assert all(d is not None for d in diffs), diffs


def test_check_patterns_fails_the_toy_and_passes_the_correct_function(monkeypatch):
    """check_patterns goes through poisoned(), which patches the package's modules: plant the toy on one of them."""
    toy = _toy_module()
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4) + 1.0
    for name in ("correct", "leaves_one_element"):
        fn = types.FunctionType(getattr(toy, name).__code__, sol_amd.ops.__dict__)      # the toy's code with ops' globals
        if name == "correct":
            poison.check_patterns(monkeypatch, lambda: fn(x), name)
        else:
            with pytest.raises(AssertionError, match="changes the result.*word 11 of 12"):
                poison.check_patterns(monkeypatch, lambda: fn(x), name)
    assert sol_amd.ops.torch is torch


def test_same_bits_compares_nans_by_bits_and_recurses():
    nan1 = torch.tensor([float("nan"), 1.0], dtype=torch.float32)
    nan2 = nan1.clone()
    assert poison.same_bits(nan1, nan2)                          # (nan != nan as floats)
    nan2.view(torch.int32)[0] = 0x7FC00001                        # another NaN payload
    assert not poison.same_bits(nan1, nan2)
    assert not poison.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    a = (torch.ones(3, dtype=torch.float32), [torch.zeros(2, dtype=torch.int64)], {"iterations": torch.tensor([3, 4], dtype=torch.int32), "converged": True, "n": 2})
    b = poison.snapshot(a)
    assert poison.same_bits(a, b)
    b[2]["iterations"][1] = 5
    assert "['iterations']" in poison.first_difference(a, b) and "word 1 of 2" in poison.first_difference(a, b)
    assert not poison.same_bits((torch.ones(3),), (torch.ones(3), torch.ones(1)))
    assert not poison.same_bits(torch.ones(3, dtype=torch.float32), torch.ones(3, dtype=torch.float64))
    assert not poison.same_bits({"converged": True}, {"converged": False})
    assert poison.same_bits(None, None) and not poison.same_bits(None, torch.ones(1))
