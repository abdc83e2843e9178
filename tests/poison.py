"""Poisoned scratch and output buffers (tests/test_poison_cpu.py, tests/test_gpu_poison.py).  A plain module: importing it touches
no device.

The package allocates every workspace and every output with torch.empty / torch.empty_like.  Under pytest such a buffer holds zeros
(a fresh segment) or what the previous call of the same shape left there (the caching allocator hands the block back) -- usually the
right answer.  A kernel that reads scratch before it writes it, or that leaves an output element unwritten, passes every oracle
comparison and every run-twice test that way.  `poisoned(monkeypatch, pattern)` replaces the name `torch` in every sol_amd module
that calls an uninitialised allocator by a stand-in whose empty / empty_like return the real allocation with every 32-bit word set
to `pattern`; everything else (zeros, full, ones, ...: where the product asks for a value it states a requirement) is the real torch.
A correct entry point returns the same bits under every pattern."""
import contextlib
import importlib

import torch

# The patterns are conditions, not tunables.
ZERO = 0x00000000           # what a fresh allocation usually gives: the baseline
ALL_ONES = 0xFFFFFFFF       # fp32 NaN; int32 and int64 -1
FLT_MAX = 0x7F7FFFFF        # finite: survives fmaxf and `<` filters; as an absmax word it silently wrecks a scale
ONE = 0x00000001            # a denormal, and a "non-zero flag"
PATTERNS = (ZERO, ALL_ONES, FLT_MAX, ONE)

UNINITIALISED = ("empty", "empty_like")     # the uninitialised allocators the package calls (test_poison_cpu.py walks its sources)
# every sol_amd module that calls one of them (test_poison_cpu.py: a module missing here fails the suite).  The command-line programs
# under scripts/ are no modules of the package (no __init__.py; they run as __main__ and import each other by bare name), so no
# stand-in can be installed on them: scripts/karman_train.py allocates the batch staging buffers of its own main() with torch.empty
# and fills each by copy before the trainer reads it.
MODULES = ("_lib", "burgers", "dist", "karman", "karman3d", "ops", "schedule2d", "schedule3d", "trainer")


def fill_(t, pattern):
    """Every 32-bit word of t's storage span := pattern (little endian), through a uint8 view: any dtype, any byte count (a tail
    shorter than a word gets the pattern's leading bytes).  t must be contiguous in some memory format (torch.empty's results are)."""
    n = t.numel() * t.element_size()
    if n == 0:
        return t
    flat = t.detach().as_strided((t.numel(),), (1,)).view(torch.uint8)
    n4 = n // 4 * 4
    if n4 and flat.data_ptr() % 4 == 0:         # whole words: one fill on the tensor's own device
        flat[:n4].view(torch.int32).fill_(pattern - (1 << 32) if pattern >> 31 else pattern)
    else:
        n4 = 0
    for k in range(n4, n):                      # (a tail shorter than a word, or an unaligned view: byte by byte)
        flat[k] = (pattern >> (8 * (k % 4))) & 0xFF
    return t


class TorchProxy:
    """Stands in for the torch module: every attribute is the real one, except the uninitialised allocators."""

    def __init__(self, pattern):
        self.__dict__["_pattern"] = int(pattern) & 0xFFFFFFFF
        self.__dict__["filled"] = 0             # allocations this stand-in filled
        self.__dict__["in_capture"] = 0         # allocations it handed through unfilled, inside a stream capture

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)

    def _poison(self, t):
        # a fill inside a stream capture would add a node the library's graph check refuses: leave the allocation as it is
        if t.is_cuda and torch.cuda.is_current_stream_capturing():
            self.__dict__["in_capture"] += 1
            return t
        self.__dict__["filled"] += 1
        return fill_(t, self._pattern)

    def empty(self, *a, **k):
        return self._poison(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._poison(torch.empty_like(*a, **k))


def modules():
    """The sol_amd modules of MODULES, imported"""
    return [importlib.import_module("sol_amd." + m) for m in MODULES]


def poisoned(monkeypatch, pattern):
    """Install the stand-in on every module of MODULES (undone with the monkeypatch).  Global torch, conftest.py and the pytest
    settings stay as they are.  -> the stand-in"""
    proxy = TorchProxy(pattern)
    for mod in modules():
        monkeypatch.setattr(mod, "torch", proxy)
    return proxy


@contextlib.contextmanager
def pattern(monkeypatch, p):
    """with pattern(monkeypatch, p): ... -- the stand-in for the block only"""
    with monkeypatch.context() as m:
        yield poisoned(m, p)


# ---------------------------------------------------------------------------------------------
# comparing results by bits
# ---------------------------------------------------------------------------------------------
def _int_view(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1).to(torch.uint8)


def first_difference(a, b, path="result"):
    """None when a and b hold the same bits, else a string naming the first place they differ.  Tensors compare through integer
    views (NaNs by their bits); tuples, lists and dicts (a CG info dict with its `iterations` and `converged` included) recurse;
    anything else compares with ==."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
            return "%s: %s against %s" % (path, type(a).__name__, type(b).__name__)
        if a.shape != b.shape or a.dtype != b.dtype:
            return "%s: %s %s against %s %s" % (path, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape))
        va, vb = _int_view(a), _int_view(b)
        ne = (va != vb).nonzero()
        if ne.numel() == 0:
            return None
        byte = int(ne[0])
        w = byte // 4 * 4
        word = lambda v: int.from_bytes(bytes(v[w:w + 4].tolist()), "little")
        return "%s: first differs at 32-bit word %d of %d (element %d): 0x%08X against 0x%08X" % (
            path, byte // 4, (va.numel() + 3) // 4, byte // a.element_size(), word(va), word(vb))
    if isinstance(a, dict) and isinstance(b, dict):
        if sorted(a, key=str) != sorted(b, key=str):
            return "%s: keys %s against %s" % (path, sorted(a, key=str), sorted(b, key=str))
        for k in sorted(a, key=str):
            r = first_difference(a[k], b[k], "%s[%r]" % (path, k))
            if r:
                return r
        return None
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        if len(a) != len(b):
            return "%s: %d entries against %d" % (path, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            r = first_difference(x, y, "%s[%d]" % (path, i))
            if r:
                return r
        return None
    return None if (a is b or a == b) else "%s: %r against %r" % (path, a, b)


def same_bits(a, b):
    return first_difference(a, b) is None


def _words(t):
    """the aligned 32-bit words of a floating tensor as int32 (None for anything else: -1 and 1 are honest integers)"""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64) or t.numel() == 0:
        return None
    return t.detach().contiguous().cpu().reshape(-1).view(torch.int32)


def leaked_pattern(got, base, path="result"):
    """None, or a string naming the first fp32 / fp64 output of `got` that holds a NaN or the FLT_MAX word where the zero-pattern
    result `base` holds none (a poison word that reached an output without changing any other bit could only hide here if `base`
    itself held one)."""
    if isinstance(got, dict):
        for k in sorted(got, key=str):
            r = leaked_pattern(got[k], base[k], "%s[%r]" % (path, k))
            if r:
                return r
        return None
    if isinstance(got, (tuple, list)):
        for i, (x, y) in enumerate(zip(got, base)):
            r = leaked_pattern(x, y, "%s[%d]" % (path, i))
            if r:
                return r
        return None
    wg, wb = _words(got), _words(base)
    if wg is None or wb is None:
        return None
    if bool(torch.isnan(got).any()) and not bool(torch.isnan(base).any()):
        return "%s: holds a NaN, the zero-pattern run holds none" % path
    fm = FLT_MAX
    if bool((wg == fm).any()) and not bool((wb == fm).any()):
        return "%s: holds the FLT_MAX word at word %d, the zero-pattern run holds none" % (path, int((wg == fm).nonzero()[0]))
    return None


def snapshot(x):
    """a deep copy of a result (tensors cloned to the host) so a later call cannot overwrite it"""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().clone()
    if isinstance(x, dict):
        return {k: snapshot(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(snapshot(v) for v in x)
    return x


def check_patterns(monkeypatch, run, what, patterns=PATTERNS):
    """run() under each pattern (objects are constructed inside run, so they allocate under the pattern too); every result must equal
    the zero-pattern run's bit for bit and must hold no NaN / FLT_MAX word that run lacks.  run returns a tensor or a (nested)
    tuple / list / dict of results; a dict's keys name the results in the failure message."""
    base = None
    for p in patterns:
        with pattern(monkeypatch, p) as proxy:
            got = snapshot(run())
        assert proxy.filled > 0, "%s: the run allocated nothing through the stand-in, so nothing was tested" % what
        if base is None:
            assert p == ZERO
            base = got
            continue
        diff = first_difference(got, base, what)
        assert diff is None, "scratch / output pattern 0x%08X changes the result -- %s" % (p, diff)
        leak = leaked_pattern(got, base, what)
        assert leak is None, "pattern 0x%08X -- %s" % (p, leak)
    return base
