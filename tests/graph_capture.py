"""Capture of the library's device entry points into a hipGraph, for the GPU tests (a helper module, not a fixture file).

INTEGRATION.md ("Graph capture"): every device entry point can be captured as it is, given one eager call of the largest batch on the
capturing stream first -- the per-(device, stream) scratch and work slabs then never have to grow while the stream captures.

capture(fn, stream) makes that eager call of `fn` on `stream`, synchronizes, captures `fn` on the same stream with
torch.cuda.CUDAGraph(keep_graph=True) and returns a Captured: the graph, the outputs the captured call returned (they are rewritten by
every replay) and the graph's node counts by type, read through hipGraphGetNodes / hipGraphNodeGetType of torch's own libamdhip64 --
the runtime instance the library is bound to (generalized_rbda_amd/__init__.py, lib()).

Lifetime rules, followed by every test that uses this module:
  * a graph is dropped and its stream synchronized before plan.release_work(), and before any larger eager call on the same stream:
    both free a slab the graph holds;
  * a graph whose capture was refused is never replayed (capture() raises, and the partial graph is dropped inside it);
  * replays take new inputs IN PLACE (copy_ into the tensors the captured call read); an entry point that changes its input
    (project_positions) has the input refilled before every replay.
"""
import ctypes
import os
from dataclasses import dataclass, field

import torch

# hipGraphNodeType (hip_runtime_api.h)
NODE_KERNEL, NODE_MEMCPY, NODE_MEMSET = 0, 1, 2

_hip = None


def hip_runtime():
    """torch's libamdhip64.so (already loaded by `import torch`: dlopen hands back the same instance)"""
    global _hip
    if _hip is None:
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        L = ctypes.CDLL(path if os.path.exists(path) else "libamdhip64.so")
        L.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        L.hipGraphGetNodes.restype = ctypes.c_int
        L.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        L.hipGraphNodeGetType.restype = ctypes.c_int
        _hip = L
    return _hip


def node_counts(graph: "torch.cuda.CUDAGraph") -> dict:
    """{"kernel": n, "memset": n, "memcpy": n, "other": n, "total": n} of a graph captured with keep_graph=True"""
    L = hip_runtime()
    handle = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    rc = L.hipGraphGetNodes(handle, None, ctypes.byref(n))
    assert rc == 0, f"hipGraphGetNodes: {rc}"
    nodes = (ctypes.c_void_p * max(n.value, 1))()
    rc = L.hipGraphGetNodes(handle, nodes, ctypes.byref(n))
    assert rc == 0, f"hipGraphGetNodes: {rc}"
    out = {"kernel": 0, "memset": 0, "memcpy": 0, "other": 0, "total": n.value}
    for i in range(n.value):
        k = ctypes.c_int(-1)
        rc = L.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(k))
        assert rc == 0, f"hipGraphNodeGetType: {rc}"
        out[{NODE_KERNEL: "kernel", NODE_MEMSET: "memset", NODE_MEMCPY: "memcpy"}.get(k.value, "other")] += 1
    return out


@dataclass
class Captured:
    graph: "torch.cuda.CUDAGraph"
    stream: "torch.cuda.Stream"
    outputs: object
    nodes: dict = field(default_factory=dict)

    def replay(self):
        """replay on the current stream (after the in-place input copies enqueued there) and wait for it"""
        self.graph.replay()
        torch.cuda.synchronize()
        return self.outputs

    def drop(self):
        """synchronize the stream and let the graph go (before release_work or a larger eager call on the stream)"""
        self.stream.synchronize()
        self.graph.reset()
        self.graph = None
        self.outputs = None


def capture(fn, stream=None, warm=None) -> Captured:
    """One eager call of `warm` (default: `fn`) on `stream` (default: a new one), then `fn` captured on that stream.  A refused
    capture raises what the library raised; its partial graph is reset here and never replayed."""
    if stream is None:
        stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        (warm or fn)()
    stream.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    try:
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            out = fn()
    except BaseException:
        stream.synchronize()
        g.reset()
        raise
    g.instantiate()
    return Captured(g, stream, out, node_counts(g))
