"""A census of a recorded HIP graph (include/dsp_frontend.h: dsp_graph_census): what a captured step is made of, looked at
instead of assumed.

``census(graph)`` takes a ``torch.cuda.CUDAGraph`` that was created with ``keep_graph=True`` and has finished recording, hands its
``raw_cuda_graph()`` handle -- the hipGraph_t -- to the library's host-only walk, and returns a ``Census``.  Nothing is launched
and the graph is not instantiated or replayed by this module."""
from __future__ import annotations

import ctypes as C
import dataclasses

from . import _native as nat


@dataclasses.dataclass
class Census:
    """Node counts of a recorded graph.  ``wide_memsets``: memset nodes of more than 4 bytes (what has been seen to replay wrong on
    this stack); ``widest_memset_bytes``: 0 without a memset node; ``roots`` / ``max_fanout``: 1 and 1 is a chain;
    ``kernel_names``: the kernel nodes' names as the runtime gives them ('?' where it gives none)."""
    nodes: int
    kernels: int
    memsets: int
    memcpys: int
    others: int
    wide_memsets: int
    widest_memset_bytes: int
    roots: int
    max_fanout: int
    kernel_names: tuple

    @property
    def is_chain(self):
        return self.roots == 1 and self.max_fanout <= 1

    def kernels_named(self, part):
        """The kernel names that contain ``part`` ('?': the kernels the runtime gave no name for)."""
        return tuple(n for n in self.kernel_names if (n == '?' if part == '?' else part in n))

    def torch_reductions(self):
        """The kernel nodes that are torch's reductions: ``at::native::reduce_kernel<...>``, whatever the shape and the operation
        (the names are the runtime's, mangled or not).  The library's own ``*_reduce_kernel`` launches -- a fixed-order sum per
        thread, no counter, no memset -- are not meant."""
        return tuple(n for n in self.kernel_names if 'reduce_kernel' in n and ('at6native' in n or 'at::native' in n))


def census_of_handle(handle):
    """The census of a raw hipGraph_t given as an integer address."""
    lib = nat.load()
    out = nat.GraphCensus()
    nat.check_value(lib.dsp_graph_census(handle, C.byref(out), None, 0), 'census: invalid graph handle')
    buf = C.create_string_buffer(max(int(out.names_bytes), 1))
    nat.check_value(lib.dsp_graph_census(handle, C.byref(out), C.cast(buf, C.c_void_p), len(buf)), 'census: invalid graph handle')
    names = tuple(n for n in buf.value.decode(errors='replace').split('\n') if n)
    return Census(nodes=out.n_nodes, kernels=out.n_kernel, memsets=out.n_memset, memcpys=out.n_memcpy, others=out.n_other,
                  wide_memsets=out.n_wide_memset, widest_memset_bytes=int(out.widest_memset_bytes), roots=out.n_roots,
                  max_fanout=out.max_fanout, kernel_names=names)


def census(graph):
    """``graph``: a ``torch.cuda.CUDAGraph(keep_graph=True)`` after its recording has ended -> ``Census``."""
    try:
        handle = graph.raw_cuda_graph()
    except (AttributeError, RuntimeError) as e:
        raise RuntimeError('census needs a torch.cuda.CUDAGraph created with keep_graph=True whose recording has ended') from e
    return census_of_handle(int(handle))
