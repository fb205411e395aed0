"""Dirty-memory harness: the product hands its kernels torch.empty memory (whatever the caching allocator returns: the previous
step's activations and gradients), the kernel tests hand them zeros.  A tile that a kernel never writes, a `beta == 0` path that
still multiplies its destination, or an output that is read before it is written all read as "0" in a zeroed buffer -- exactly
what the reference expects there.  The helpers here run ONE launch three times, on destinations pre-filled with

    ZERO   zeros,
    NAN    the quiet-NaN bit pattern of the dtype,
    JUNK   a large finite value no test data contains (0xA5 bytes for integer outputs),

and require bit-identical results: the kernels are deterministic (the fp64 loss accumulators, which are atomics, excepted --
those are *state* and are compared to rtol 1e-12 by the tests that own them).

A plain module, like tests/philox_ref.py; no fixture, no pytest setting.
"""
import inspect

import torch

ZERO, NAN, JUNK = "ZERO", "NAN", "JUNK"
FILLS = (ZERO, NAN, JUNK)

_QNAN = {torch.float32: 0x7FC00000, torch.float64: 0x7FF8000000000000, torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}
# a finite value no test tensor holds; the 16-bit types narrow it (bf16 has fp32's exponent range, fp16 tops out at 65504)
_JUNK = {torch.float32: 1.2345e30, torch.float64: 1.2345e30, torch.bfloat16: 1.2345e30, torch.float16: 60000.0}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """The tensor's storage as integers of the element size (flat, contiguous, on the CPU): NaN == NaN iff the bits match."""
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.view(_INT_VIEW[t.element_size()]).reshape(-1)


def fill_(t, fill):
    """Pre-fill `t` in place (views included: only the elements the view addresses are touched)."""
    if t.numel() == 0:
        return t
    if fill == ZERO:
        t.zero_()
    elif t.dtype in _QNAN:
        if fill == NAN:
            pattern = torch.tensor([_QNAN[t.dtype]], dtype=torch.int64).to(_INT_VIEW[t.element_size()]).view(t.dtype)
            t.copy_(pattern.to(t.device).expand(t.numel()).reshape(t.shape))
        else:
            t.fill_(_JUNK[t.dtype])
    else:           # uint8 / integer plain outputs: 0xA5 bytes for both non-zero fills
        word = int.from_bytes(b"\xa5" * t.element_size(), "little", signed=False)
        if t.dtype != torch.uint8 and word >= 1 << (8 * t.element_size() - 1):
            word -= 1 << (8 * t.element_size())
        t.fill_(bool(word) if t.dtype == torch.bool else word)
    return t


def _tensors(a):
    """The tensors an argument carries: itself, the `.t` of an ops.Planes, or the members of a list / tuple / dict."""
    if torch.is_tensor(a):
        return [a]
    if hasattr(a, "t") and torch.is_tensor(getattr(a, "t")):
        return [a.t]
    if isinstance(a, (list, tuple)):
        return [t for x in a for t in _tensors(x)]
    if isinstance(a, dict):
        return [t for x in a.values() for t in _tensors(x)]
    return []


def _fresh(a, device):
    """A private copy of an argument (on `device` when given); non-tensor arguments are passed through."""
    if torch.is_tensor(a):
        return a.detach().clone() if device is None else a.detach().to(device, copy=True)
    if hasattr(a, "t") and torch.is_tensor(getattr(a, "t")):
        c = object.__new__(type(a))
        c.t = _fresh(a.t, device)
        return c
    if isinstance(a, (list, tuple)):
        return type(a)(_fresh(x, device) for x in a)
    if isinstance(a, dict):
        return {k: _fresh(v, device) for k, v in a.items()}
    return a


def _arg_names(backend, name, n):
    """Parameter names of the call, for messages: of the callable itself (minus its `backend` parameter), else of the first
    class in the backend's MRO that defines `name` with a spelled-out signature (EmuBackend wraps some methods in *args)."""
    cands = [name] if callable(name) else [c.__dict__[name] for c in type(backend).__mro__ if name in c.__dict__]
    for fn in cands:
        try:
            ps = list(inspect.signature(fn).parameters.values())
        except (TypeError, ValueError):
            continue
        if any(p.kind == p.VAR_POSITIONAL for p in ps):
            continue
        params = [p.name for p in ps if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)][1:]   # drop self / backend
        return [params[i] if i < len(params) else f"arg{i}" for i in range(n)]
    return [f"arg{i}" for i in range(n)]


def first_diff(a, b):
    """First flat index at which two tensors differ bit for bit, or None."""
    ba, bb = bits(a), bits(b)
    if ba.shape != bb.shape:
        return 0
    ne = (ba != bb).nonzero()
    return int(ne[0]) if ne.numel() else None


def run_dirty(backend, name, args, outs, scratch=(), state=(), untouched=None, device=None, names=None, kwargs=None,
              on_fill=None):
    """Call ``backend.<name>(*args)`` once per fill on fresh copies of `args` (moved to `device` when given).

    outs      indices of the arguments the call must WRITE: pre-filled with the fill, returned, compared by assert_same_bits;
    scratch   indices of workspaces: pre-filled with the fill, neither returned nor compared;
    state     indices of arguments with a documented initial value (counters, tickets, running statistics, accumulators): they
              keep the value passed in, may change, and are returned under their names next to the outputs;
    untouched {index in outs: bool mask, the argument's shape} -- the part of an output the header documents as left alone: it
              must still hold the fill after the call (it is zeroed in what is returned, so the fills compare equal there).
    Every other tensor argument is an input: it must be bitwise unchanged after the call.  `name` may be a callable
    ``fn(backend, *args)`` for a launch that needs its arguments assembled (expert tables of views, keyword arguments).
    `on_fill(fill)` is called in front of each run (a PoisonTorch that follows the fill: the workspaces the backend allocates)."""
    fn = name if callable(name) else getattr(backend, name)
    label = getattr(name, "__name__", str(name))
    names = list(names) if names is not None else _arg_names(backend, name, len(args))
    untouched = dict(untouched or {})
    runs = {}
    for fill in FILLS:
        if on_fill is not None:
            on_fill(fill)
        call = [_fresh(a, device) for a in args]
        for i in list(outs) + list(scratch):
            for t in _tensors(call[i]):
                fill_(t, fill)
        before = {i: [t.clone() for t in _tensors(a)] for i, a in enumerate(call)
                  if i not in state and i not in scratch and (i not in outs or i in untouched)}
        if callable(name):
            name(backend, *call, **(kwargs or {}))
        else:
            fn(*call, **(kwargs or {}))
        if device is not None and torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        got = {}
        for i, a in enumerate(call):
            ts = _tensors(a)
            if i in outs or i in state:
                for k, t in enumerate(ts):
                    key = names[i] if len(ts) == 1 else f"{names[i]}[{k}]"
                    t = t.detach().cpu().clone()
                    if i in untouched:
                        mask = untouched[i].reshape(t.shape).cpu()
                        was = before[i][k].cpu()
                        d = first_diff(torch.where(mask, t, was), was)
                        assert d is None, (f"{label}: `{key}` was written at flat index {d}, inside the region documented as "
                                           f"left untouched ({fill} fill)")
                        t = torch.where(mask, torch.zeros_like(t), t)
                    got[key] = t
            elif i not in scratch:
                for k, (t, was) in enumerate(zip(ts, before[i])):
                    key = names[i] if len(ts) == 1 else f"{names[i]}[{k}]"
                    d = first_diff(t, was)
                    assert d is None, f"{label}: read-only input `{key}` was modified at flat index {d} ({fill} fill)"
        runs[fill] = got
    return runs


def assert_same_bits(runs, approx=(), rtol=1e-12, what=""):
    """The outputs of the three fills agree bit for bit and hold no NaN.  Names in `approx` (fp64 sums that atomics add in any
    order) are compared with `rtol` instead.  A failure names the tensor and the first differing flat index."""
    ref = runs[ZERO]
    for fill, got in runs.items():
        assert got.keys() == ref.keys()
        for key, t in got.items():
            if t.is_floating_point():
                nan = torch.isnan(t.float() if t.dtype != torch.float64 else t).reshape(-1).nonzero()
                assert nan.numel() == 0, (f"{what}`{key}` holds a NaN at flat index {int(nan[0])} of {t.numel()} "
                                          f"(shape {tuple(t.shape)}) after the run on {fill}-filled destinations")
            if key in approx:
                assert torch.allclose(t.double(), ref[key].double(), rtol=rtol, atol=0.0), \
                    f"{what}`{key}` differs between the ZERO and the {fill} fill beyond rtol {rtol}"
                continue
            d = first_diff(t, ref[key])
            assert d is None, (f"{what}`{key}` differs between the ZERO and the {fill} fill at flat index {d} of {t.numel()} "
                               f"(shape {tuple(t.shape)}): {t.reshape(-1)[d].item()!r} against {ref[key].reshape(-1)[d].item()!r}")


class PoisonTorch:
    """Stands in for the `torch` name of ONE module (monkeypatch.setattr(module, "torch", PoisonTorch(fill)) on mmdyn_hip.ops,
    .layers, .engine -- never on torch itself): every attribute is the real one, except that empty / empty_like return
    floating-point tensors pre-filled with the fill.  The synchronise orders the fill before a consumer on another stream."""

    def __init__(self, fill, real=torch):
        object.__setattr__(self, "_fill", fill)
        object.__setattr__(self, "_real", real)

    def __getattr__(self, k):
        return getattr(self._real, k)

    def set_fill(self, fill):
        object.__setattr__(self, "_fill", fill)

    def _poison(self, t):
        if t.is_floating_point():
            fill_(t, self._fill)
            if t.is_cuda:
                self._real.cuda.synchronize()
        return t

    def empty(self, *a, **k):
        return self._poison(self._real.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._poison(self._real.empty_like(*a, **k))
