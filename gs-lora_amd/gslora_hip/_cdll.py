"""The loading code of every ctypes binding here (_lib.py and the five _lib_<x>.py), once: a library that is opened on first use, checked
against its binding's signatures, and never replaced by a fallback; and the three helpers the tensor-level wrappers share. torch is imported
only by _stream(), on its first call.
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
