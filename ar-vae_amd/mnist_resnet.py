"""MnistResNet: the ResNet-18 digit classifier of the Morpho-MNIST evaluation, inference only, on the HIP kernels.

Surface of the reference's imagevae/mnist_resnet.py:7-19: a torchvision ResNet-18 (BasicBlock, [2, 2, 2, 2], 10 classes) whose
stem takes one channel and whose average pool is AvgPool2d(1) (the identity at 28 x 28, where layer4's map is 1 x 1); forward returns
softmax probabilities.  The state_dict has torchvision's 122 keys and shapes, so the checkpoint the reference publishes
(MnistRESNET.pt) loads unchanged; torchvision itself is not needed.  The modules below only HOLD the tensors: the arithmetic
is csrc/resnet18.hip (batch-norm folded into the convolutions in float64, three-term bf16 MFMA products, 22 launches).

Batch-norm runs in evaluation mode only (running statistics, eps 1e-5): a forward in training mode raises.
"""
import torch
from torch import nn

from . import _lib, ops
from .model import Model

BN_EPS = 1e-5
LAYER_CHANNELS = (64, 128, 256, 512)
LAYER_INPUT_HW = (7, 7, 4, 2)                  # side of the map each layer receives at 28 x 28 input


def fold_batch_norm(weight, gamma, beta, mean, var, eps=BN_EPS):
    """(w', b') with conv(x, w') + b' == BatchNorm2d.eval()(conv(x, w)): w' = w gamma / sqrt(var + eps), b' = beta - mean gamma /
    sqrt(var + eps), in float64 (the arithmetic arvae_resnet18_prepare does on the device)."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return weight.double() * scale.view(-1, 1, 1, 1), beta.double() - mean.double() * scale


def live_taps(hin, hout, ksize, stride, pad):
    """taps (ky, kx) that read a pixel inside a hin x hin input for at least one of the hout x hout output pixels"""
    live = [k for k in range(ksize) if any(0 <= o * stride - pad + k < hin for o in range(hout))]
    return [(ky, kx) for ky in live for kx in live]


class _Block(nn.Module):
    """torchvision's BasicBlock as a tensor holder: conv1, bn1, conv2, bn2 [, downsample.0, downsample.1]"""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout, eps=BN_EPS)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout, eps=BN_EPS)
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout, eps=BN_EPS))
        else:
            self.downsample = None


def _bn(bn):
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var)


class MnistResNet(Model):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64, eps=BN_EPS)
        cin = 64
        for i, cout in enumerate(LAYER_CHANNELS):
            stride = 1 if i == 0 else 2
            setattr(self, f'layer{i + 1}', nn.Sequential(_Block(cin, cout, stride), _Block(cout, cout, 1)))
            cin = cout
        self.fc = nn.Linear(512, 10)
        self.trainer_config = ''
        self.update_filepath()
        self._prep = None
        self._prep_key = None

    def __repr__(self):
        return 'MnistRESNET'

    # -- the 19 convolutions after the stem, in the library's order ---------------------------------------------------------
    def conv_sequence(self):
        """[(geometry, conv module, bn module, role)] with role in 'conv1' | 'downsample' | 'conv2'"""
        seq = []
        for i, cout in enumerate(LAYER_CHANNELS):
            hin = LAYER_INPUT_HW[i]
            for b, block in enumerate(getattr(self, f'layer{i + 1}')):
                cin = block.conv1.in_channels
                stride = block.conv1.stride[0]
                g1 = ops.ResnetConv(hin, cin, cout, 3, stride)
                seq.append((g1, block.conv1, block.bn1, 'conv1'))
                if block.downsample is not None:
                    seq.append((ops.ResnetConv(hin, cin, cout, 1, stride), block.downsample[0], block.downsample[1], 'downsample'))
                seq.append((ops.ResnetConv(g1.hout, cout, cout, 3, 1), block.conv2, block.bn2, 'conv2'))
                hin = g1.hout
        return seq

    def _state_tensors(self):
        return [t for k, t in self.state_dict(keep_vars=True).items() if not k.endswith('num_batches_tracked')]

    def _check_runnable(self, x):
        if self.training:
            raise RuntimeError('MnistResNet runs batch-norm in evaluation mode only (running statistics): call .eval() before the '
                               'forward; training the classifier is outside this build')
        if not x.is_cuda or not self.fc.weight.is_cuda:
            raise RuntimeError('MnistResNet runs on the GPU only (HIP kernels, no CPU fallback): call .cuda() on the model and the input')

    def prepared(self):
        """the library's prepared block (folded, split weights), rebuilt whenever a tensor of the state was replaced, moved or
        changed in place (data_ptr / _version of every entry, as FusedImageVAE and the tick decoder watch theirs)"""
        tensors = self._state_tensors()
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if self._prep is None or key != self._prep_key:
            for t in tensors:
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise TypeError('MnistResNet needs contiguous float32 weights')
            w = _lib.ResnetWeights()
            w.stem_w = self.conv1.weight.data_ptr()
            for j, t in enumerate(_bn(self.bn1)):
                w.stem_bn[j] = t.data_ptr()
            for i, (_, conv, bn, _) in enumerate(self.conv_sequence()):
                w.conv_w[i] = conv.weight.data_ptr()
                w.bn_w[i], w.bn_b[i], w.bn_mean[i], w.bn_var[i] = (t.data_ptr() for t in _bn(bn))
            w.fc_w, w.fc_b = self.fc.weight.data_ptr(), self.fc.bias.data_ptr()
            self._prep = ops.resnet18_prepare(w, self.fc.weight.device)
            self._prep_key = key
        return self._prep

    def classify(self, x):
        """x (B, 1, 28, 28) float32 on the device -> (logits (B, 10), probabilities (B, 10), argmax (B,) int64); one library call"""
        self._check_runnable(x)
        with torch.no_grad():
            return ops.resnet18_forward(self.prepared(), x.detach().contiguous())

    def forward(self, x):
        return self.classify(x)[1]

    def predict(self, x):
        """argmax labels (int64, lowest index on an exact tie) from the head kernel"""
        return self.classify(x)[2]

    def forward_layerwise(self, x):
        """the same network through the per-layer entry points, one prepared block per layer (tools/time_digit_acc.py takes its
        per-launch split from here; the results are bit-identical to classify's)"""
        self._check_runnable(x)
        with torch.no_grad():
            h = ops.resnet18_maxpool(ops.resnet18_stem(ops.resnet18_stem_prepare(self.conv1.weight.detach(), _bn(self.bn1)),
                                                       x.detach().contiguous()))
            identity = h
            for geom, conv, bn, role in self.conv_sequence():
                prep = ops.resnet18_conv_prepare(geom, conv.weight.detach(), _bn(bn))
                if role == 'conv1':
                    block_in, identity = h, h
                    h = ops.resnet18_conv(geom, prep, h, relu=True)
                elif role == 'downsample':
                    identity = ops.resnet18_conv(geom, prep, block_in)
                else:
                    h = ops.resnet18_conv(geom, prep, h, residual=identity, relu=True)
            return ops.resnet18_head(self.fc.weight.detach(), self.fc.bias.detach(), h.view(h.shape[0], 512))
