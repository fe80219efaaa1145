"""The digit classifier restated in plain torch (nn.Conv2d / BatchNorm2d / max_pool2d under torchvision's ResNet-18 key names) and
the random fixture the classifier tests share.  Built from the architecture (a 7x7 stride-2 stem on one channel, max-pool 3x3
stride 2, four layers of two basic blocks at 64 / 128 / 256 / 512 channels, AvgPool2d(1), fc 512 -> 10); not product code, no test
in here.

The fixture: weights from numpy.random.RandomState(seed), never torch's generator, made at test time (44 MB: too big to commit).
Conv weights He-normal (fan-out); BN weight U(0.5, 1.5), bias and running mean N(0, 0.2), running var U(0.5, 1.5); inputs sparse
random strokes in [0, 1]; then the head is CENTRED on the test batch: fc.weight ~ N scaled so that the logits of the centred
features have unit spread, fc.bias = -fc.weight . mean_feature (float64).  Without the centring a random ResNet predicts one
class for every input and an argmax comparison shows nothing."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

CHANNELS = (64, 128, 256, 512)


class Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(out)) + identity)


class ResNetRef(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for i, cout in enumerate(CHANNELS):
            setattr(self, f'layer{i + 1}', nn.Sequential(Block(cin, cout, 1 if i == 0 else 2), Block(cout, cout, 1)))
            cin = cout
        self.fc = nn.Linear(512, 10)

    def features(self, x):
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return torch.flatten(x, 1)              # AvgPool2d(1, stride=1) of a 1 x 1 map is the identity

    def forward(self, x):
        """logits"""
        return self.fc(self.features(x))


def expected_shapes():
    """the 122 state_dict entries of the checkpoint, in torchvision's order"""
    def bn(prefix, c):
        return [(f'{prefix}.weight', (c,)), (f'{prefix}.bias', (c,)), (f'{prefix}.running_mean', (c,)), (f'{prefix}.running_var', (c,)),
                (f'{prefix}.num_batches_tracked', ())]
    out = [('conv1.weight', (64, 1, 7, 7))] + bn('bn1', 64)
    cin = 64
    for i, cout in enumerate(CHANNELS):
        for b in range(2):
            p = f'layer{i + 1}.{b}'
            c_in = cin if b == 0 else cout
            out += [(f'{p}.conv1.weight', (cout, c_in, 3, 3))] + bn(f'{p}.bn1', cout)
            out += [(f'{p}.conv2.weight', (cout, cout, 3, 3))] + bn(f'{p}.bn2', cout)
            if b == 0 and i > 0:
                out += [(f'{p}.downsample.0.weight', (cout, cin, 1, 1))] + bn(f'{p}.downsample.1', cout)
        cin = cout
    return out + [('fc.weight', (10, 512)), ('fc.bias', (10,))]


def stroke_images(n, seed):
    """(n, 1, 28, 28) float32 in [0, 1]: a few random line strokes per image, most pixels zero"""
    rs = np.random.RandomState(seed)
    x = np.zeros((n, 1, 28, 28), np.float32)
    t = np.linspace(0.0, 1.0, 40)
    for i in range(n):
        for _ in range(rs.randint(2, 5)):
            p0, p1 = rs.uniform(3, 25, 2), rs.uniform(3, 25, 2)
            ys = np.rint(p0[0] + t * (p1[0] - p0[0])).astype(int)
            xs = np.rint(p0[1] + t * (p1[1] - p0[1])).astype(int)
            x[i, 0, ys, xs] = np.maximum(x[i, 0, ys, xs], rs.uniform(0.3, 1.0, t.size).astype(np.float32))
    return x


def random_state_dict(seed):
    """fp32 tensors under the 122 keys (fc not yet centred: centre_head)"""
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape in expected_shapes():
        if key.endswith('num_batches_tracked'):
            v = np.array(1000, np.int64)
        elif key.endswith('running_var'):
            v = rs.uniform(0.5, 1.5, shape)
        elif key.endswith('running_mean') or (key.endswith('.bias') and 'bn' in key or key.endswith('downsample.1.bias')):
            v = rs.normal(0.0, 0.2, shape)
        elif len(shape) == 4:
            v = rs.normal(0.0, np.sqrt(2.0 / (shape[0] * shape[2] * shape[3])), shape)
        elif key == 'fc.weight':
            v = rs.normal(0.0, 1.0, shape)
        elif key == 'fc.bias':
            v = np.zeros(shape)
        else:                                   # BN weight
            v = rs.uniform(0.5, 1.5, shape)
        sd[key] = torch.from_numpy(np.asarray(v, np.int64 if key.endswith('num_batches_tracked') else np.float32))
    return sd


def centre_head(sd, x):
    """rescale fc.weight and set fc.bias so that the float64 logits of the batch x have zero mean and unit spread per class"""
    net = build(sd, torch.float64)
    with torch.no_grad():
        feat = net.features(torch.from_numpy(x).double())
        mean = feat.mean(0)
        w = sd['fc.weight'].double()
        w = w / ((feat - mean) @ w.t()).std()
        sd['fc.weight'] = w.float()
        sd['fc.bias'] = (-(sd['fc.weight'].double() @ mean)).float()
    return sd


def build(sd, dtype):
    """the restatement in evaluation mode holding sd (fp32 values) in `dtype`"""
    net = ResNetRef()
    net.load_state_dict(sd)
    return net.to(dtype).eval()


class Fixture:
    """state dict, inputs, and the float64 / torch-fp32 CPU results every whole-network test compares against (computed once)"""

    def __init__(self, n=67, seed=7):          # seed 7, 67 images: all ten classes, no float64 top-2 margin under 8e-2
        self.x = stroke_images(n, seed + 1)
        self.sd = centre_head(random_state_dict(seed), self.x)
        self.refresh()

    def refresh(self):
        with torch.no_grad():
            xt = torch.from_numpy(self.x)
            self.logits64 = build(self.sd, torch.float64)(xt.double())
            self.logits32 = build(self.sd, torch.float32)(xt)
        self.probs64 = torch.softmax(self.logits64, 1)
        self.probs32 = torch.softmax(self.logits32, 1)
        self.pred64 = self.logits64.argmax(1)
        top2 = self.logits64.topk(2, 1).values
        self.margin64 = top2[:, 0] - top2[:, 1]
        self.logit_err32 = float((self.logits32.double() - self.logits64).abs().max())


def rel_l2(a, ref):
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    return float((a - ref).norm() / ref.norm())


def check_predictions(pred, logits64_rows, logit_err32, max_unclear=0.05):
    """rule 3 of the whole-network test: equal to the float64 argmax on every row whose float64 top-2 margin exceeds 100 x the
    torch-fp32 max logit error; at most 5 % of the rows may fall under that margin"""
    top2 = logits64_rows.topk(2, 1).values
    clear = (top2[:, 0] - top2[:, 1]) > 100.0 * logit_err32
    assert float((~clear).float().mean()) <= max_unclear, f'{int((~clear).sum())} of {len(clear)} rows under the margin'
    want = logits64_rows.argmax(1)
    assert torch.equal(pred.cpu()[clear], want[clear])
    return clear
