"""features/classifier.py::_DynEnc against what the reference's layers.DynamicEncoder produced on the CPU
(tests/golden/bigru_golden.npz), and the routing between its nn.GRU path and the native one where no GPU is present."""
import numpy as np
import pytest

import bigru_cases as bc


@pytest.fixture(scope='module')
def g():
    return bc.load_golden()


@pytest.mark.parametrize('tag', bc.TAGS)
def test_the_gru_path_reproduces_the_reference_encoder_on_cpu(tag, g):
    import torch
    enc = bc.encoder(g, tag)
    x, lens, _ = bc.maker().inputs(tag, np)
    with torch.no_grad():
        y, hn = enc.run(torch.from_numpy(x), lens, native=False)
        assert torch.equal(enc(torch.from_numpy(x), lens), y)              # the default on a CPU tensor is the same path
    worst = bc.deviation(g, tag, y.numpy(), hn.numpy())
    print(f'{tag}: worst deviation / scale = {worst:.3g}')
    assert worst <= bc.BAR
    n = torch.from_numpy(lens)
    assert all(float(y[int(n[b]):, b].abs().max()) == 0.0 for b in range(len(lens)) if int(n[b]) < y.shape[0])


def test_native_supported_names_the_reason_for_a_cpu_tensor(g):
    import torch
    enc = bc.encoder(g, 'c')
    why = enc.native_supported(torch.zeros(9, 5, 13))
    assert isinstance(why, str) and 'not on a GPU' in why


def test_native_true_on_a_cpu_tensor_raises(g):
    import torch
    enc = bc.encoder(g, 'c')
    x, lens, _ = bc.maker().inputs('c', np)
    with torch.no_grad(), pytest.raises(RuntimeError, match='not on a GPU'):
        enc(torch.from_numpy(x), lens, native=True)
    with pytest.raises(RuntimeError, match='gradient'):
        enc(torch.from_numpy(x), lens, native=True)


def test_heads_take_native_enc_and_keep_their_parameter_names():
    import inspect
    import torch
    from features import classifier as C
    rg = np.load(bc.os.path.join(bc.HERE, 'golden', 'rnn_golden.npz'))
    torch.manual_seed(0)
    head = C.RNNHead().eval()
    assert C.fill_parameters(head, int(rg['seed'])) == [str(n) for n in rg['names']]
    assert [n for n, _ in head.named_parameters()][:4] == ['enc.gru.weight_ih_l0', 'enc.gru.weight_hh_l0', 'enc.gru.bias_ih_l0',
                                                          'enc.gru.bias_hh_l0']
    assert list(head.state_dict()) == [n for n, _ in head.named_parameters()]           # the handle is no buffer
    for cls in (C.RNNHead, C.HRNNHead, C.HRNNAttHead, C.TransformerHead, C.HMRNNHead):
        assert 'native_enc' in inspect.signature(cls.forward).parameters, cls.__name__
    inp = torch.from_numpy(rg['inp'][:, :2])
    with torch.no_grad():
        assert torch.equal(head(inp, rg['len0'][:2], native_enc=False), head(inp, rg['len0'][:2]))
        with pytest.raises(RuntimeError):
            head(inp, rg['len0'][:2], native_enc=True)


def test_the_emulation_of_the_kernels_layout_reproduces_the_reference(g):
    """tools/bigru_emul.py restates csrc/kernels_bigru.h in numpy (packed weights, operand layout, masking, direction sum):
    the index arithmetic and the semantics of the kernel hold against the real class without a GPU."""
    import importlib.util
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('_bigru_emul', bc.os.path.join(ROOT, 'tools', 'bigru_emul.py'))
    emul = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(emul)
    enc = bc.encoder(g, 'c')
    x, lens, _ = bc.maker().inputs('c', np)
    I, H, L = (int(v) for v in g['c_shape'])
    y, hn = emul.encoder(x, lens, [p.detach().numpy() for p in enc._params()], I, H, L)
    assert bc.deviation(g, 'c', y, hn) <= bc.BAR
    assert not y.view(np.uint32)[3:, 0].any()                                  # exact zero rows behind column 0's three steps
