"""The digit classifier without a GPU: checkpoint surface, BN folding, live-tap packing, the trainer's guards and the C-ABI's
host side (the library builds with hipcc on a CPU-only machine)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import arvae_amd  # noqa: E402,F401
import resnet_ref  # noqa: E402
from arvae_amd import mnist_resnet  # noqa: E402
from arvae_amd.mnist_resnet import MnistResNet  # noqa: E402

# the checkpoint's layout, written out: 122 entries
BN = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')
CONVS = {'conv1.weight': (64, 1, 7, 7),
         'layer1.0.conv1.weight': (64, 64, 3, 3), 'layer1.0.conv2.weight': (64, 64, 3, 3),
         'layer1.1.conv1.weight': (64, 64, 3, 3), 'layer1.1.conv2.weight': (64, 64, 3, 3),
         'layer2.0.conv1.weight': (128, 64, 3, 3), 'layer2.0.conv2.weight': (128, 128, 3, 3), 'layer2.0.downsample.0.weight': (128, 64, 1, 1),
         'layer2.1.conv1.weight': (128, 128, 3, 3), 'layer2.1.conv2.weight': (128, 128, 3, 3),
         'layer3.0.conv1.weight': (256, 128, 3, 3), 'layer3.0.conv2.weight': (256, 256, 3, 3), 'layer3.0.downsample.0.weight': (256, 128, 1, 1),
         'layer3.1.conv1.weight': (256, 256, 3, 3), 'layer3.1.conv2.weight': (256, 256, 3, 3),
         'layer4.0.conv1.weight': (512, 256, 3, 3), 'layer4.0.conv2.weight': (512, 512, 3, 3), 'layer4.0.downsample.0.weight': (512, 256, 1, 1),
         'layer4.1.conv1.weight': (512, 512, 3, 3), 'layer4.1.conv2.weight': (512, 512, 3, 3)}
NORMS = {'bn1': 64, 'layer1.0.bn1': 64, 'layer1.0.bn2': 64, 'layer1.1.bn1': 64, 'layer1.1.bn2': 64,
         'layer2.0.bn1': 128, 'layer2.0.bn2': 128, 'layer2.0.downsample.1': 128, 'layer2.1.bn1': 128, 'layer2.1.bn2': 128,
         'layer3.0.bn1': 256, 'layer3.0.bn2': 256, 'layer3.0.downsample.1': 256, 'layer3.1.bn1': 256, 'layer3.1.bn2': 256,
         'layer4.0.bn1': 512, 'layer4.0.bn2': 512, 'layer4.0.downsample.1': 512, 'layer4.1.bn1': 512, 'layer4.1.bn2': 512}
# the seven geometries of the 19 convolutions (+ the 1x1 stride-2 downsamples): (hin, hout, ksize, stride, pad) -> live taps
GEOMETRIES = {(7, 7, 3, 1, 1): 9, (7, 4, 3, 2, 1): 9, (4, 4, 3, 1, 1): 9, (4, 2, 3, 2, 1): 9, (2, 2, 3, 1, 1): 9, (2, 1, 3, 2, 1): 4,
              (1, 1, 3, 1, 1): 1, (7, 4, 1, 2, 0): 1, (4, 2, 1, 2, 0): 1, (2, 1, 1, 2, 0): 1}


def table():
    shapes = dict(CONVS)
    for prefix, c in NORMS.items():
        for name in BN:
            shapes[f'{prefix}.{name}'] = () if name == 'num_batches_tracked' else (c,)
    shapes['fc.weight'], shapes['fc.bias'] = (10, 512), (10,)
    return shapes


@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_state_dict_is_torchvisions_resnet18():
    sd = MnistResNet().state_dict()
    want = table()
    assert len(want) == 122 and len(sd) == 122
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(sd.keys()) == [k for k, _ in resnet_ref.expected_shapes()]            # torchvision's order
    assert all(tuple(s) == want[k] for k, s in resnet_ref.expected_shapes())
    assert not any('bias' in k for k in sd if 'conv' in k or 'downsample.0' in k)     # no convolution has a bias
    assert sd['bn1.num_batches_tracked'].dtype == torch.int64


def test_repr_filepath_and_round_trip(tmp_path, monkeypatch):
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(tmp_path))
    model = MnistResNet()
    assert repr(model) == 'MnistRESNET' and model.trainer_config == ''
    assert model.filepath == os.path.join(str(tmp_path), 'MnistRESNET', 'MnistRESNET.pt')
    sd = resnet_ref.random_state_dict(5)
    os.makedirs(os.path.dirname(model.filepath))
    torch.save(sd, model.filepath)                      # a checkpoint as the reference writes it: a bare state_dict
    model.load(cpu=True)
    got = model.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    model.save()
    again = torch.load(model.filepath, map_location='cpu')
    assert list(again.keys()) == list(sd.keys()) and all(torch.equal(again[k], sd[k]) for k in sd)
    bad = dict(sd)
    del bad['layer3.0.downsample.1.running_var']
    with pytest.raises(RuntimeError, match='running_var'):
        model.load_state_dict(bad)


def test_training_mode_and_cpu_tensors_are_refused():
    model = MnistResNet()
    x = torch.zeros(2, 1, 28, 28)
    with pytest.raises(RuntimeError, match='evaluation mode only'):
        model.train()(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        model.eval()(x)


def test_bn_fold_in_float64_reproduces_eval_batchnorm():
    rs = np.random.RandomState(11)
    for cout, cin, k, stride, pad in ((16, 8, 3, 1, 1), (12, 8, 3, 2, 1), (8, 4, 1, 2, 0), (6, 1, 7, 2, 3)):
        w = torch.from_numpy(rs.normal(0, 0.3, (cout, cin, k, k)))
        gamma, var = torch.from_numpy(rs.uniform(0.5, 1.5, cout)), torch.from_numpy(rs.uniform(0.05, 2.0, cout))
        beta, mean = torch.from_numpy(rs.normal(0, 0.5, cout)), torch.from_numpy(rs.normal(0, 0.5, cout))
        x = torch.from_numpy(rs.normal(0, 1, (3, cin, 9, 9)))
        bn = torch.nn.BatchNorm2d(cout, eps=1e-5).double().eval()
        with torch.no_grad():
            bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(mean), bn.running_var.copy_(var)
            want = bn(F.conv2d(x, w, None, stride, pad))
        wf, bf = mnist_resnet.fold_batch_norm(w, gamma, beta, mean, var)
        got = F.conv2d(x, wf, bf, stride, pad)
        assert wf.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


def brute_force_live(hin, hout, k, stride, pad):
    live = set()
    for oy in range(hout):
        for ox in range(hout):
            for ky in range(k):
                for kx in range(k):
                    if 0 <= oy * stride - pad + ky < hin and 0 <= ox * stride - pad + kx < hin:
                        live.add(ky * k + kx)
    return sorted(live)


def test_live_tap_table_matches_brute_force(lib):
    from arvae_amd import ops
    for (hin, hout, k, stride, pad), count in GEOMETRIES.items():
        want = brute_force_live(hin, hout, k, stride, pad)
        assert len(want) == count, (hin, hout, k, stride)
        assert [ky * k + kx for ky, kx in mnist_resnet.live_taps(hin, hout, k, stride, pad)] == want
        for cin, cout in ((64, 64), (256, 512)):
            g = ops.ResnetConv(hin, cin, cout, k, stride)
            assert (g.hout, g.pad) == (hout, pad)
            assert ops.resnet18_live_taps(g) == want                               # what the library packs
            d = g.desc()
            assert lib.arvae_resnet18_conv_prep_floats(ctypes.byref(d)) == cout * count * cin * 3 // 2 + cout
    # the network's own sequence uses exactly these geometries, and only the centre tap anywhere in layer4 after its first conv
    seq = MnistResNet().conv_sequence()
    assert len(seq) == 19
    assert {(g.hin, g.hout, g.ksize, g.stride, g.pad) for g, _, _, _ in seq} == set(GEOMETRIES)
    assert [len(ops.resnet18_live_taps(g)) for g, _, _, _ in seq[14:]] == [4, 1, 1, 1, 1]
    for g, conv, bn, _ in seq:
        assert tuple(conv.weight.shape) == (g.cout, g.cin, g.ksize, g.ksize) and bn.num_features == g.cout


def test_entries_are_declared_exported_and_sized(lib):
    from arvae_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'arvae_hip.h')).read(), flags=re.S)
    names = ['arvae_resnet18_prep_floats', 'arvae_resnet18_prepare', 'arvae_resnet18_ws_floats', 'arvae_resnet18_forward',
             'arvae_resnet18_conv', 'arvae_resnet18_conv_prepare', 'arvae_resnet18_conv_prep_floats', 'arvae_resnet18_live_taps',
             'arvae_resnet18_stem', 'arvae_resnet18_stem_prepare', 'arvae_resnet18_stem_prep_floats', 'arvae_resnet18_maxpool',
             'arvae_resnet18_head']
    for name in names:
        assert len(re.findall(r'\b%s\s*\(' % name, text)) == 1, f'{name}: declared once'
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.arvae_abi_version() == 16
    prep = lib.arvae_resnet18_prep_floats()
    # every live weight as three bf16 terms (1.5 floats) + the biases + the fp32 stem and head: 1/9 of layer4's 3x3 taps remain
    live = 4 * 64 * 64 * 9 + 64 * 128 * 10 + 3 * 128 * 128 * 9 + 128 * 256 * 10 + 3 * 256 * 256 * 9 + 256 * 512 * 5 + 3 * 512 * 512
    biases = 4 * 64 + 5 * 128 + 5 * 256 + 5 * 512
    assert prep == live * 3 // 2 + biases + (49 * 64 + 64) + (10 * 512 + 12) and prep % 4 == 0
    for n in (1, 3, 67, 128, 1280):
        ws = lib.arvae_resnet18_ws_floats(n)
        assert ws == n * (14 * 14 * 64 + 4 * 7 * 7 * 64) and ws > 0 and ws % 4 == 0
    assert lib.arvae_resnet18_stem_prep_floats() == 49 * 64 + 64
    assert lib.arvae_resnet18_ws_floats(0) == -1 and b'batch' in lib.arvae_last_error_string()
    # argument checks are host code: nothing is launched
    assert lib.arvae_resnet18_forward(None, None, 4, None, None, None, None, None) == -1
    assert b'null pointer' in lib.arvae_last_error_string()
    assert lib.arvae_resnet18_prepare(None, None, None) == -1
    bad = _lib.ResnetConvDesc(7, 7, 48, 7, 7, 64, 3, 1, 1, 0)
    assert lib.arvae_resnet18_conv_prep_floats(ctypes.byref(bad)) == -1 and b'geometry' in lib.arvae_last_error_string()
    bad = _lib.ResnetConvDesc(7, 7, 64, 5, 5, 64, 3, 1, 1, 0)                      # output extent does not follow from the input's
    assert lib.arvae_resnet18_live_taps(ctypes.byref(bad), None) == -1


def test_ctypes_structs_match_the_header(tmp_path):
    import shutil
    import subprocess
    from arvae_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('gcc not available')
    src = tmp_path / 'sizes.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s/include/arvae_hip.h"\nint main(void) {\n'
                   'printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(arvae_resnet18_conv_t), sizeof(arvae_resnet18_weights_t),\n'
                   'offsetof(arvae_resnet18_weights_t, conv_w), offsetof(arvae_resnet18_weights_t, bn_var), '
                   'offsetof(arvae_resnet18_weights_t, fc_b));\nreturn 0; }\n' % ROOT)
    exe = tmp_path / 'sizes'
    subprocess.run([gcc, '-o', str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    w = _lib.ResnetWeights
    assert got == [ctypes.sizeof(_lib.ResnetConvDesc), ctypes.sizeof(w), w.conv_w.offset, w.bn_var.offset, w.fc_b.offset]


class DspritesDataset:
    pass


class MorphoMnistDataset:
    pass


def test_trainer_guards(tmp_path, monkeypatch):
    from arvae_amd.image_vae import DspritesVAE, MnistVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(tmp_path))
    assert ImageVAETrainer(DspritesDataset(), DspritesVAE()).get_resnet_accuracy() is None
    trainer = ImageVAETrainer(MorphoMnistDataset(), MnistVAE())
    with pytest.raises(FileNotFoundError, match='MnistRESNET.pt') as err:
        trainer.get_resnet_accuracy()
    assert os.path.join(str(tmp_path), 'MnistRESNET', 'MnistRESNET.pt') in str(err.value) and 'Downloading Models' in str(err.value)
    pred, gt = torch.tensor([1, 2, 3, 4]), torch.tensor([1, 2, 0, 4])
    assert float(ImageVAETrainer.mean_accuracy_pred(pred, gt)) == 0.75
