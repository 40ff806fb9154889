"""The census of a recorded graph on the GPU (include/dsp_frontend.h: dsp_graph_census; features/graphcheck.py).  Two small graphs
are recorded with ``torch.cuda.CUDAGraph(keep_graph=True)`` and looked at; NEITHER IS REPLAYED (the first holds a memset node of
256 bytes, which is the very thing that has been seen to replay wrong on this stack), nor instantiated.

  * a ``dsp_memset`` of 256 bytes and one library kernel: one memset node, the widest 256 bytes, flagged as wide; one kernel;
  * two library kernels on one stream: 2 kernel nodes, 1 root, fan-out 1 -- a chain --, no memset node;
  * the kernel names are the runtime's, newline-separated in the C result: both carry the library kernel's name;
  * a recorded ``a.sum(0).sum(0)`` and ``a.sum()`` of torch's: ``Census.torch_reductions()`` recognises their kernels by the names
    the runtime gives (this is what the gate of ``TrainBatch.capture`` outside its table relies on), and none is nameless."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu


def _record(body):
    """Record ``body(stream handle)`` on a side stream into a kept graph -> (graph, whatever the launches touch)."""
    import torch
    from features import _native as nat
    nat.require_device()
    lib = nat.load()
    dev = torch.device('cuda', 0)
    nbytes = nat.c_i64(0)
    nat.check(lib.dsp_metrics_bytes(4, 0, C.byref(nbytes)))
    state = torch.zeros(nbytes.value // 4, dtype=torch.int32, device=dev)
    target = torch.zeros(64, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=side):
        body(lib, nat, side.cuda_stream, state, target)
    return graph, (state, target)


def test_memset_of_256_bytes_is_counted_and_flagged():
    from features.graphcheck import census

    def body(lib, nat, stream, state, target):
        nat.check(lib.dsp_memset(target.data_ptr(), 0, 256, stream))
        nat.check(lib.dsp_metrics_reset(state.data_ptr(), 4, 0, stream))
    graph, hold = _record(body)
    c = census(graph)                                                  # the graph is looked at, never replayed
    assert (c.memsets, c.wide_memsets, c.widest_memset_bytes) == (1, 1, 256), c
    assert (c.kernels, c.memcpys, c.others, c.nodes) == (1, 0, 0, 2), c
    assert c.is_chain and (c.roots, c.max_fanout) == (1, 1), c
    assert len(c.kernel_names) == 1 and c.kernels_named('xent_reset_kernel') == c.kernel_names, c
    assert c.kernels_named('reduce_kernel') == () and c.torch_reductions() == ()
    del graph, hold


def test_two_library_kernels_are_a_chain_without_a_memset():
    from features import _native as nat
    from features.graphcheck import census, census_of_handle

    def body(lib, nat_, stream, state, target):
        nat_.check(lib.dsp_metrics_reset(state.data_ptr(), 4, 0, stream))
        nat_.check(lib.dsp_metrics_reset(state.data_ptr(), 4, 0, stream))
    graph, hold = _record(body)
    c = census(graph)
    assert (c.kernels, c.memsets, c.wide_memsets, c.widest_memset_bytes, c.memcpys, c.others) == (2, 0, 0, 0, 0, 0), c
    assert (c.roots, c.max_fanout) == (1, 1) and c.is_chain, c
    assert len(c.kernel_names) == 2 and all('xent_reset_kernel' in n for n in c.kernel_names), c
    # the C entry with a names buffer too small for the second name: whole names only, and the size all of them need
    lib = nat.load()
    out = nat.GraphCensus()
    first = len(c.kernel_names[0])
    buf = C.create_string_buffer(first + 2 + 3)
    nat.check(lib.dsp_graph_census(int(graph.raw_cuda_graph()), C.byref(out), C.cast(buf, C.c_void_p), len(buf)))
    assert buf.value.decode() == c.kernel_names[0] + '\n'
    assert out.names_bytes == sum(len(n) + 1 for n in c.kernel_names) + 1 and out.n_kernel == 2
    assert census_of_handle(int(graph.raw_cuda_graph())) == c
    with pytest.raises(ValueError, match='NULL graph'):
        census_of_handle(0)
    del graph, hold


def test_torch_reductions_are_recognised_by_name():
    import torch
    from features.graphcheck import census
    dev = torch.device('cuda', 0)
    a = torch.ones(200, 64, 200, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        a.sum(0).sum(0), a.sum()                                       # (warm: nothing is allocated or compiled while recording)
    side.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=side):
        keep = (a.sum(0).sum(0), a.sum(), a * 2.0)
    c = census(graph)                                                  # looked at, never replayed
    print(f'torch sums: {c.kernels} kernels, {c.memsets} memsets (widest {c.widest_memset_bytes} B), names {c.kernel_names}')
    assert c.kernels >= 4 and c.kernels_named('?') == ()
    assert len(c.torch_reductions()) >= 3 and len(c.torch_reductions()) < c.kernels      # the elementwise kernel is not one
    del graph, keep
