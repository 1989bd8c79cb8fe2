"""NaN-poisoned, red-zoned allocations for tests.

``guarded(device)`` replaces ``torch.empty`` / ``empty_like`` / ``zeros`` /
``zeros_like`` and ``Tensor.new_empty`` / ``new_zeros`` while it is active. A
request on ``device`` that carries only ``dtype`` / ``device`` arguments is
served from one uint8 block of ``RED + roundup(nbytes, 256) + RED`` bytes filled
with byte 0xFF; the caller gets the contiguous view of the middle. 0xFF repeated
is a NaN in fp32, f16, bf16 and f64 and -1 / 255 in the integer types, so an
element a kernel never wrote, or a load past the end that feeds a result, cannot
pass as a plausible number. ``check()`` reports every allocation whose
surroundings no longer hold 0xFF, with the site that made it.

What it cannot see: a store more than RED bytes away from a tensor, memory the
native library obtains without going through Python, and anything another
process allocates. It observes only: the zones lie inside the same allocation
as the tensor, so an overrun it can catch lands in memory the process owns.

This is an ordinary module that tests import; it is no pytest plugin.
"""
import ast
import contextlib
import os
import sys

import torch

RED = 4096
ALIGN = 256
FILL = 0xFF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "fastvocoder_amd")

_MODULE_FNS = ("empty", "empty_like", "zeros", "zeros_like")
_TENSOR_FNS = ("new_empty", "new_zeros")
_HERE = os.path.abspath(__file__)


class Site(tuple):
    """(file, line, function) of the frame that asked for an allocation."""
    __slots__ = ()

    def __new__(cls, file, line, function):
        return super().__new__(cls, (file, line, function))

    file = property(lambda s: s[0])
    line = property(lambda s: s[1])
    function = property(lambda s: s[2])

    def __str__(self):
        return f"{os.path.relpath(self.file, ROOT) if self.file.startswith(ROOT) else self.file}:{self.line} in {self.function}"


class Allocation:
    __slots__ = ("block", "view", "nbytes", "site", "kind")

    def __init__(self, block, view, nbytes, site, kind):
        self.block, self.view, self.nbytes, self.site, self.kind = block, view, nbytes, site, kind

    def __repr__(self):
        return f"<{self.kind} {tuple(self.view.shape)} {self.view.dtype} at {self.site}>"


class PassThrough:
    __slots__ = ("site", "kind", "device", "reason")

    def __init__(self, site, kind, device, reason):
        self.site, self.kind, self.device, self.reason = site, kind, device, reason

    def __repr__(self):
        return f"<{self.kind} on {self.device} passed through ({self.reason}) at {self.site}>"


def _site(depth):
    f = sys._getframe(depth)
    # a helper of this module (place) asks on behalf of its own caller
    while os.path.abspath(f.f_code.co_filename) == _HERE and f.f_back is not None:
        f = f.f_back
    return Site(os.path.abspath(f.f_code.co_filename), f.f_lineno, f.f_code.co_name)


def _roundup(n, a):
    return (n + a - 1) // a * a


def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def _dense(t):
    """Non-overlapping and dense: some permutation of the dimensions is contiguous."""
    expect = 1
    for stride, size in sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1):
        if stride != expect:
            return False
        expect *= size
    return True


class Guard:
    def __init__(self, device):
        self.device = torch.device(device)
        self.allocations = []
        self.passed = []
        self._orig = {}

    # ---- the allocator -------------------------------------------------------------------
    def _same_device(self, dev):
        dev = torch.device(dev)
        if dev.type != self.device.type:
            return False
        if dev.type != "cuda":
            return True
        cur = torch.cuda.current_device()
        return (cur if dev.index is None else dev.index) == (cur if self.device.index is None else self.device.index)

    def _alloc(self, shape, dtype, device, site, kind, zero):
        esize = torch._utils._element_size(dtype)
        n = 1
        for s in shape:
            n *= s
        nbytes = n * esize
        block = self._orig["empty"](RED + _roundup(nbytes, ALIGN) + RED, dtype=torch.uint8, device=device)
        block.fill_(FILL)
        view = block[RED:RED + nbytes].view(dtype).view(shape)
        if zero:
            view.zero_()
        self.allocations.append(Allocation(block, view, nbytes, site, kind))
        return view

    def _serve(self, kind, orig, args, kwargs, shape, dtype, device, extra, site, zero):
        """Guard the request, or hand it to the original and record why."""
        reason = None
        if extra:
            reason = "keyword arguments " + ", ".join(sorted(extra))
        elif not self._same_device(device):
            reason = "other device"
        if reason is not None:
            self.passed.append(PassThrough(site, kind, torch.device(device), reason))
            return orig(*args, **kwargs)
        return self._alloc(shape, dtype, device, site, kind, zero)

    def _make_plain(self, kind, zero):
        orig = self._orig[kind]

        def fn(*size, **kwargs):
            site = _site(2)
            kw = dict(kwargs)
            if "size" in kw and not size:
                size = (kw.pop("size"),)
            dtype = kw.pop("dtype", None)
            device = kw.pop("device", None)
            dtype = torch.get_default_dtype() if dtype is None else dtype
            device = torch.get_default_device() if device is None else device
            return self._serve(kind, orig, size, kwargs, _shape_of(size) if not kw else None, dtype, device, kw, site, zero)
        fn.__name__ = kind
        return fn

    def _make_like(self, kind, zero):
        orig = self._orig[kind]

        def fn(src, **kwargs):
            site = _site(2)
            kw = dict(kwargs)
            dtype = kw.pop("dtype", None)
            device = kw.pop("device", None)
            # preserve_format on a contiguous source asks for exactly what the guard returns
            mf = kw.get("memory_format")
            if mf is not None and (mf is torch.contiguous_format or (mf is torch.preserve_format and src.is_contiguous())):
                kw.pop("memory_format")
            # torch keeps the strides of a permuted dense source; of any other it returns a contiguous tensor, as the guard does
            if not kw and not src.is_contiguous() and _dense(src):
                kw["(strides of a permuted source)"] = True
            dtype = src.dtype if dtype is None else dtype
            device = src.device if device is None else device
            return self._serve(kind, orig, (src,), kwargs, tuple(src.shape), dtype, device, kw, site, zero)
        fn.__name__ = kind
        return fn

    def _make_new(self, kind, zero):
        orig = self._orig[kind]

        def fn(src, *size, **kwargs):
            site = _site(2)
            kw = dict(kwargs)
            if "size" in kw and not size:
                size = (kw.pop("size"),)
            dtype = kw.pop("dtype", None)
            device = kw.pop("device", None)
            dtype = src.dtype if dtype is None else dtype
            device = src.device if device is None else device
            return self._serve(kind, orig, (src,) + tuple(size), kwargs, _shape_of(size) if not kw else None, dtype, device, kw,
                               site, zero)
        fn.__name__ = kind
        return fn

    # ---- patching ------------------------------------------------------------------------
    def _install(self):
        for name in _MODULE_FNS:
            self._orig[name] = getattr(torch, name)
        for name in _TENSOR_FNS:
            self._orig[name] = getattr(torch.Tensor, name)
        self._own = {name: name in torch.Tensor.__dict__ for name in _TENSOR_FNS}
        torch.empty = self._make_plain("empty", False)
        torch.zeros = self._make_plain("zeros", True)
        torch.empty_like = self._make_like("empty_like", False)
        torch.zeros_like = self._make_like("zeros_like", True)
        torch.Tensor.new_empty = self._make_new("new_empty", False)
        torch.Tensor.new_zeros = self._make_new("new_zeros", True)

    def _remove(self):
        for name in _MODULE_FNS:
            setattr(torch, name, self._orig[name])
        for name in _TENSOR_FNS:
            if self._own[name]:
                setattr(torch.Tensor, name, self._orig[name])
            else:
                delattr(torch.Tensor, name)          # inherited from the C base class again

    # ---- what tests call -----------------------------------------------------------------
    def place(self, t):
        """A copy of ``t`` in a guarded block of its own (on the guard's device)."""
        site = _site(2)
        view = self._alloc(tuple(t.shape), t.dtype, self.device, site, "place", False)
        view.copy_(t.detach())
        return view

    @staticmethod
    def poison(t):
        """Refill a live contiguous tensor with 0xFF bytes."""
        assert t.is_contiguous(), "poison() needs a contiguous tensor"
        if t.numel():
            t.detach().reshape(-1).view(torch.uint8).fill_(FILL)
        return t

    def check(self):
        """The allocations whose red zones no longer hold 0xFF everywhere."""
        if not self.allocations:
            return []
        counts = []
        for a in self.allocations:
            front, back = a.block[:RED], a.block[RED + a.nbytes:]
            counts.append((front != FILL).sum() + (back != FILL).sum())
        counts = torch.stack(counts).cpu().tolist()
        return [a for a, c in zip(self.allocations, counts) if c]

    def sites(self):
        return [a.site for a in self.allocations]

    def unguarded(self, under=PACKAGE, device_type=None):
        """Pass-through requests made from a file under ``under`` for ``device_type``
        (the guard's own by default)."""
        kind = self.device.type if device_type is None else device_type
        return [p for p in self.passed if p.site.file.startswith(under + os.sep) and p.device.type == kind]


@contextlib.contextmanager
def guarded(device):
    g = Guard(device)
    g._install()
    try:
        yield g
    finally:
        g._remove()


poison = Guard.poison


# ---- static site list ---------------------------------------------------------------------
class StaticSite(tuple):
    """(relative file, first line, last line, column, call name, enclosing function)"""
    __slots__ = ()
    file = property(lambda s: s[0])
    line = property(lambda s: s[1])
    end_line = property(lambda s: s[2])
    col = property(lambda s: s[3])
    call = property(lambda s: s[4])
    function = property(lambda s: s[5])

    def __str__(self):
        return f"{self.file}:{self.line} {self.call} in {self.function}"


def scan_sites(package=PACKAGE):
    """Every ``torch.empty/empty_like/zeros/zeros_like(...)`` and ``.new_empty/.new_zeros(...)``
    call in the package's Python files, in file and line order."""
    out = []
    for dirpath, dirnames, filenames in sorted(os.walk(package)):
        dirnames[:] = sorted(d for d in dirnames if d != "__pycache__")
        for fn in sorted(filenames):
            if not fn.endswith(".py"):
                continue
            path = os.path.join(dirpath, fn)
            with open(path) as f:
                tree = ast.parse(f.read(), path)
            rel = os.path.relpath(path, ROOT)

            def visit(node, func):
                if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                    func = node.name
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute):
                    a = node.func
                    if (a.attr in _MODULE_FNS and isinstance(a.value, ast.Name) and a.value.id == "torch") or a.attr in _TENSOR_FNS:
                        out.append(StaticSite((rel, node.lineno, node.end_lineno, node.col_offset, a.attr, func)))
                for child in ast.iter_child_nodes(node):
                    visit(child, func)
            visit(tree, "<module>")
    return sorted(out)


def reached(static, sites):
    """The members of ``static`` that one of the recorded ``sites`` (of allocations or of
    pass-throughs) lies on. Two calls on one line count as reached together."""
    lines = {}
    for s in sites:
        if s.file.startswith(ROOT + os.sep):
            lines.setdefault(os.path.relpath(s.file, ROOT), set()).add(s.line)
    return [s for s in static if any(s.line <= n <= s.end_line for n in lines.get(s.file, ()))]
