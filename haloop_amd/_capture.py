"""HIP graph capture of a host-sync-free chain of launches, stated once for the inference paths (the decoders and the encoder of
transformer.py, generation.Sampler, streaming, infer.py).  train.py's captures differ in substance and stay written out there."""
import torch


def capture(fn):
    """Run ``fn()`` once on a side stream (the warm-up: whatever it builds lazily, such as weight images, is built outside the capture),
    wait for it, then capture the same call.  -> (graph, the captured call's return value)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


class GraphCache:
    """Captured graphs of one module's launches by key, at most 8 (the oldest goes first).  An entry is captured again when a parameter
    of the module has changed (the graph replays launches that read weight images built from the old values)."""
    LIMIT = 8

    def __init__(self):
        self.entries = {}

    def entry(self, module, key, static, fn):
        """The entry of ``key``: ``graph``, ``static`` (the tensors ``static()`` returned, which the graph reads: refill them, then
        replay) and ``outs`` (what ``fn(static)`` returned under capture, which a replay overwrites: clone them)."""
        stamp = tuple((p._version, p.data_ptr()) for p in module.parameters())
        entry = self.entries.get(key)
        if entry is None or entry['stamp'] != stamp:
            st = static()
            graph, outs = capture(lambda: fn(st))
            # the graph reads the cached weight images by address: keep them alive as long as the graph
            held = [list(m._images._cache.values()) for m in module.modules() if hasattr(m, '_images')] + [getattr(module, '_dec_images', None)]
            if len(self.entries) >= self.LIMIT:
                self.entries.pop(next(iter(self.entries)))
            entry = dict(stamp=stamp, graph=graph, static=st, outs=outs, held=held)
            self.entries[key] = entry
        return entry
