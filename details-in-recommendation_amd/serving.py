"""serving.py -- HIP-graph replay of a model forward for the reference's own batch sizes.

The reference trains/evaluates at batch 100 / 256 (models/DeepCrossNetwork/train.py:16-17).  At that size the
forward is a chain of ~10 short launches (gather+FM, linear term, rocBLAS GEMMs, elementwise) and is bound by launch
latency, not by HBM.  `GraphedForward` captures one forward into a HIP graph (torch.cuda.CUDAGraph = hipGraph on
ROCm; the kernels of libdir_hip.so are launched on torch's current stream, so they are captured like any other
node) and replays it on static input / output buffers.
"""
import torch


class GraphedForward:
    def __init__(self, fn, *example_inputs, warmup=3, frozen_weights=False):
        """fn(*tensors) -> tensor; example_inputs fix the shapes.  Inputs are copied into static buffers at call.

        Default capture: every per-version cache is bypassed inside the capture (the pack kernels are part of the graph), so a replay
        follows in-place weight updates -- except DeepFM's packed serving rows, a copy of the whole tables: the capture reads them as
        they are, records the tensors they were copied from (ops.capture_hold), and a call after one of those was modified in place
        (or after ops.invalidate_caches()) captures again before it replays.  static_out is then a new tensor.
        frozen_weights: capture under ops.frozen_weights() -- the graph reads the weight images the warm-up calls built instead of
        re-packing them on every replay (three launches of a one-launch DeepFM forward); replays then do NOT follow later in-place
        updates of what reached the graph through a cache (weight images, packed rows, folded batch norms) while parameters a kernel
        reads itself (biases, tables outside the packed rows) are read as they are: build a new GraphedForward after loading new weights.
        Either way the cache entries the graph reads are kept alive in self.hold for the graph's lifetime: an eager call at new weights,
        ops.invalidate_caches() or a cache's size limit cannot free them under the graph."""
        self.fn, self.frozen = fn, frozen_weights
        self.static_in = [t.clone() for t in example_inputs]
        self.captures = 0
        self._capture(warmup)

    def _capture(self, warmup):
        from . import ops
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):          # fills the library's per-kernel caches, rocBLAS workspaces, TableSets
                self.fn(*self.static_in)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        hold = ops.frozen_weights() if self.frozen else ops.capture_hold()
        with hold, torch.cuda.graph(self.graph), torch.no_grad():
            self.static_out = self.fn(*self.static_in)
        self.hold = hold
        self.captures += 1

    def __call__(self, *inputs):
        for s, t in zip(self.static_in, inputs):
            s.copy_(t, non_blocking=True)
        if not self.frozen and self.hold.guarded and self.hold.moved():
            torch.cuda.current_stream().synchronize()      # the old graph's last replay is done before its pool is released
            self._capture(1)                 # a guarded cache entry is stale: one eager call rebuilds it, then capture again
        self.graph.replay()
        return self.static_out
