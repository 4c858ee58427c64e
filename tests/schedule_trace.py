"""The launch schedule of a ViTRunner pass as data (tests/test_hip_schedule_trace.py).

`ScheduleTrace` is a context manager. Inside it every public function of gslora_hip.ops is a call-through recorder; on exit the functions
are put back. One event per call: [name, {parameter: value}, result]. The arguments are bound to the function's own signature and a
parameter that holds its default is left out, so `f(x, 1.0)` and `f(x, alpha=1.0)` are one event and a keyword passed at its default
is none. Scalars, strings and None stand for themselves, a dtype / device by its name, tuples and lists element by element (the stride
pairs of the gradient-fused GEMM, the entries of lora_grad_batch). A tensor is the string

    t<label>+<storage offset>[shape][strides]<dtype>

where the label counts the storages in the order in which the trace first met them: two tensors with one label are views of one buffer.
The trace holds a reference to every tensor it has seen until it exits, so the allocator hands no address out twice inside a trace and a
label cannot come to mean two buffers. Addresses themselves are never recorded: they differ from run to run.

`ViTRunner.grad_hook` events are ["hook", i]: hook(runner) installs the recording hook, so the trace shows where _grads_done / _flush fall.

Left unwrapped: the classes, and QUERIES — host-side questions that launch and allocate nothing. (gemm_nt itself asks code() /
gemm_code() on every call, and how often the runner asks for a tile choice is not part of the schedule.)"""
import inspect
import types

import torch

QUERIES = frozenset({"code", "gemm_code", "gemm_tile_choice", "attention_kernel", "check_num_tokens", "check_lora_rank"})


def _signature(fn):
    """fn's signature; for the (*a, **kw) closure of ops._profiled, that of the function it wraps."""
    sig = inspect.signature(fn)
    if all(p.kind in (p.VAR_POSITIONAL, p.VAR_KEYWORD) for p in sig.parameters.values()):
        for cell in fn.__closure__ or ():
            inner = cell.cell_contents
            if isinstance(inner, types.FunctionType) and inner.__name__ == fn.__name__:
                return inspect.signature(inner)
    return sig


class ScheduleTrace:
    def __init__(self):
        self.events = []
        self._labels, self._keep, self._saved = {}, [], {}

    def _enc(self, v):
        if isinstance(v, torch.Tensor):
            self._keep.append(v)
            label = self._labels.setdefault(v.untyped_storage().data_ptr(), len(self._labels))
            dims = lambda xs: "[" + ",".join(str(int(x)) for x in xs) + "]"
            return f"t{label}+{v.storage_offset()}{dims(v.shape)}{dims(v.stride())}{str(v.dtype).replace('torch.', '')}"
        if isinstance(v, (tuple, list)):
            return [self._enc(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self._enc(x) for k, x in v.items()}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, (torch.dtype, torch.device)):
            return str(v).replace("torch.", "")
        return type(v).__name__

    def _recorder(self, name, fn):
        sig = _signature(fn)

        def call(*a, **kw):
            bound = sig.bind(*a, **kw)
            args = {}
            for k, v in bound.arguments.items():      # (tensors first: `==` on a tensor is no answer)
                d = sig.parameters[k].default
                if isinstance(v, torch.Tensor) or d is inspect.Parameter.empty or type(v) is not type(d) or v != d:
                    args[k] = self._enc(v)
            event = [name, args, None]
            self.events.append(event)      # before the call: the calls an ops function makes itself follow it
            out = fn(*a, **kw)
            event[2] = self._enc(out)
            return out
        return call

    def hook(self, runner):
        runner.grad_hook = lambda i: self.events.append(["hook", int(i)])

    def __enter__(self):
        from gslora_hip import ops
        for name, fn in vars(ops).items():
            if isinstance(fn, types.FunctionType) and not name.startswith("_") and name not in QUERIES and fn.__module__ == ops.__name__:
                self._saved[name] = fn
        for name, fn in self._saved.items():
            setattr(ops, name, self._recorder(name, fn))
        return self

    def __exit__(self, *exc):
        from gslora_hip import ops
        for name, fn in self._saved.items():
            setattr(ops, name, fn)
        self._saved.clear()
        self._keep.clear()
        return False
