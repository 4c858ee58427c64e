"""The loading code of every ctypes binding here (_lib.py and the five _lib_<x>.py), once: a library that is opened on first use, checked
against its binding's signatures, and never replaced by a fallback; the three helpers the tensor-level wrappers share; and what the two
entry tables of the batched kernels share (columns, table_to_device, DeviceTable). torch is imported only inside the functions that need it.
"""
import ctypes as C
import os


class LazyLib:
    """One shared library. path: a string, or a callable read at load() (a module's LIB_PATH as it stands then); signatures: name -> argtypes;
    restypes: name -> restype where it is not int; last_error: the name of the library's *_last_error; closing: the sentence that ends the
    "not found" message."""

    def __init__(self, path, signatures, restypes, last_error, closing):
        self._path, self._signatures, self._restypes, self._last_error, self._closing = path, signatures, restypes, last_error, closing
        self._lib = None

    def load(self):
        """Load the shared library (once). Raises RuntimeError — never falls back to another path."""
        if self._lib is None:
            path = self._path() if callable(self._path) else self._path
            if not os.path.exists(path):
                raise RuntimeError(
                    f"{os.path.basename(path)} not found at {path}. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    f"(hipcc --offload-arch=gfx950). {self._closing}")
            try:
                lib = C.CDLL(path)
            except OSError as e:  # missing libamdhip64 etc.
                raise RuntimeError(f"cannot load {path}: {e}") from e
            for name, argtypes in self._signatures.items():
                try:
                    fn = getattr(lib, name)
                except AttributeError as e:
                    raise RuntimeError(f"{path} does not export {name}; rebuild the extension") from e
                fn.argtypes = argtypes
                fn.restype = self._restypes.get(name, C.c_int)
            self._lib = lib
        return self._lib

    def loaded(self):
        return self._lib is not None

    def last_error(self):
        msg = getattr(self.load(), self._last_error)()
        return msg.decode() if msg else ""

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed (code {rc}): {self.last_error()}")

    def nonneg(self, n, call):
        """n, what a *_ws_elems entry point returned for `call` (its name and arguments as text): negative means refused."""
        if n < 0:
            raise RuntimeError(f"{call} refused: {self.last_error()}")
        return n


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    """The leading dimension of a 2-D view with unit column stride."""
    return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]


def columns(entries, *ctypes):
    """A list of tuples as one ctypes array per tuple position, the k-th of element type ctypes[k]: the host arrays of a *_layout call."""
    return [(ct * len(entries))(*[e[k] for e in entries]) for k, ct in enumerate(ctypes)]


def table_to_device(table, device):
    """The host table (a ctypes array of structures) as a device byte tensor, as it is."""
    import torch
    host = torch.frombuffer(bytearray(C.string_at(C.addressof(table), C.sizeof(table))), dtype=torch.uint8)
    return host.to(device)


class DeviceTable:
    """What the prepared tables of the batched kernels share (reg.RegTerms, kd.ParamDist): the entry table a *_layout call filled, uploaded
    as it is with the workspace of its forward; the data_ptr() of the tensors it points at, so that a `.loss()` can tell that one moved; and
    the views of the one flat gradient buffer the backward fills, at the table's goff. When to rebuild, and what `rebuilds` counts, is each
    class's own rule."""
    table_dev = None

    def _upload(self, table, total_blocks, watched, device):
        import torch
        self._ptrs = [t.data_ptr() for t in watched]
        self.table_dev = table_to_device(table, device)
        self.ws = torch.empty(total_blocks, device=device, dtype=torch.float32)

    def _moved(self, watched):
        return len(watched) != len(self._ptrs) or any(t.data_ptr() != q for t, q in zip(watched, self._ptrs))

    def grad_views(self, g, tensors, needs):
        """g: the flat buffer of g_elems floats; -> per tensor its view at goff, or None where no gradient is needed."""
        return tuple(g[off:off + t.numel()].view(t.shape) if need else None for off, t, need in zip(self.goffs, tensors, needs))
