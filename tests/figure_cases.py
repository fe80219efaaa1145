"""What the figure tests (test_figures.py on the CPU, test_figures_gpu.py on the GPU) share: a numpy restatement of the grid that
arvae_render_frames assembles (torchvision's make_grid) and of its two quantisers, the acceptance rule, and the case tables.

The rule.  For a logit l let v = 255 sigmoid(l) in float64 (from the fp32 logit), q the mode's quantiser (truncating: floor(v);
rounding: floor(v + 0.5); both clamped to [0, 255]) and TAU = 255 * 2^-21: eight units in the last place of a probability in
[0.5, 1), the budget of expf, one add, one reciprocal and the product.  A byte passes when it lies in [q(v - TAU), q(v + TAU)].
Where a case's inputs sit away from the quantiser's steps the byte must equal the fp32-CPU byte, torch.sigmoid(l).mul(255)
[.add(0.5)].clamp(0, 255).byte(), exactly.  The rule may leave at most MAX_UNDETERMINED of a case's pixels undetermined
(q(v - TAU) != q(v + TAU)); test_figures.py asserts that share, and that the fp32-CPU bytes pass the rule, for every case."""
import itertools

import numpy as np
import torch

TAU = 255.0 * 2.0 ** -21
MAX_UNDETERMINED = 1e-3


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def effective_padding(n_frames, cells_per_frame, padding):
    """make_grid returns a lone image unpadded (ops.render_frames keeps that)"""
    return 0 if n_frames == 1 and cells_per_frame == 1 else padding


def geometry(h, w, cells_per_frame, nrow, padding):
    """-> (xmaps, ymaps, Hg, Wg)"""
    xmaps = min(nrow, cells_per_frame)
    ymaps = -(-cells_per_frame // xmaps)
    return xmaps, ymaps, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding


def grid(images, cells, nrow, padding, pad, channels):
    """images (N, h, w) of any dtype (bytes, or the bounds of bytes), cells (F, cells_per_frame) with -1 = blank
    -> (F, Hg, Wg, channels), every channel equal, `pad` wherever no image lies"""
    images, cells = np.asarray(images), np.asarray(cells)
    _, h, w = images.shape
    n_frames, per_frame = cells.shape
    xmaps, _, hg, wg = geometry(h, w, per_frame, nrow, padding)
    out = np.full((n_frames, hg, wg), pad, dtype=images.dtype)
    for f in range(n_frames):
        for k in range(per_frame):
            if cells[f, k] < 0:
                continue
            y, x = padding + (k // xmaps) * (h + padding), padding + (k % xmaps) * (w + padding)
            out[f, y:y + h, x:x + w] = images[cells[f, k]]
    return np.repeat(out[..., None], channels, axis=3)


# ---- quantisers -----------------------------------------------------------------------------------------------------------------
def q64(v, rounding):
    """the mode's quantiser on float64 values v = 255 p"""
    return np.clip(np.floor(np.asarray(v, np.float64) + (0.5 if rounding else 0.0)), 0, 255).astype(np.uint8)


def scaled64(src, logits):
    """v = 255 sigmoid(l) (or 255 * value) in float64 from the fp32 source"""
    s = np.asarray(src, np.float32).astype(np.float64)
    with np.errstate(over='ignore'):
        return 255.0 / (1.0 + np.exp(-s)) if logits else 255.0 * s


def interval(src, logits, rounding):
    """(lowest, highest) byte the rule accepts, per element"""
    v = scaled64(src, logits)
    return q64(v - TAU, rounding), q64(v + TAU, rounding)


def fp32_cpu_bytes(src, logits, rounding):
    """the reference's own arithmetic in fp32 on the CPU"""
    t = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32))
    t = (torch.sigmoid(t) if logits else t).mul(255)
    if rounding:
        t = t.add(0.5)
    return t.clamp(0, 255).byte().numpy()


def pad_byte(pad_value, rounding):
    return int(fp32_cpu_bytes(np.array([pad_value], np.float32), False, rounding)[0])


def undetermined_share(src, logits, rounding):
    lo, hi = interval(src, logits, rounding)
    return float(np.mean(lo != hi))


# ---- quantiser cases: name -> (source (N, h, w) fp32, logits?, rounding?, the bytes expected or None) ------------------------------
def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p) - np.log1p(-p)


def quantiser_cases():
    b = np.arange(256, dtype=np.float64)
    every_trunc = np.append(_logit((b[:255] + 0.5) / 255.0), 25.0)                     # 255 p = b + 0.5: half a step from both edges
    every_round = np.concatenate(([-25.0], _logit(b[1:255] / 255.0), [25.0]))           # 255 p + 0.5 = b + 0.5
    expect = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    return {
        'every_byte_trunc': (every_trunc.astype(np.float32).reshape(1, 16, 16), True, False, expect),
        'every_byte_round': (every_round.astype(np.float32).reshape(1, 16, 16), True, True, expect),
        # sigmoid(0) = 0.5 exactly: 127.5 truncates to 127 and rounds to 128; from |l| = 20 on the byte is saturated
        'edges_trunc': (np.array([[[0.0, 20.0, -20.0, 25.0, -25.0, 88.0, -88.0, 200.0, -200.0]]], np.float32), True, False,
                        np.array([[[127, 255, 0, 255, 0, 255, 0, 255, 0]]], np.uint8)),
        'edges_round': (np.array([[[0.0, 20.0, -20.0, 25.0, -25.0, 88.0, -88.0, 200.0, -200.0]]], np.float32), True, True,
                        np.array([[[128, 255, 0, 255, 0, 255, 0, 255, 0]]], np.uint8)),
        # values taken as given, clamped outside [0, 1]
        'values_trunc': (np.array([[[-0.5, 0.0, 0.25, 0.5, 1.0, 1.5, -1e30, 1e30]]], np.float32), False, False,
                         np.array([[[0, 0, 63, 127, 255, 255, 0, 255]]], np.uint8)),
        'values_round': (np.array([[[-0.5, 0.0, 0.25, 0.5, 1.0, 1.5, -1e30, 1e30]]], np.float32), False, True,
                         np.array([[[0, 0, 64, 128, 255, 255, 0, 255]]], np.uint8)),
    }


def random_logits():
    """3 * randn(64, 1, 28, 28), seed 0: the scale at which the rule leaves under 0.1 % of the pixels undetermined (a scale of 8
    leaves 3.5 % in truncating mode: logits between 14.6 and 20 land on 254 or 255 with the sigmoid's last bit)"""
    g = torch.Generator().manual_seed(0)
    return (3.0 * torch.randn(64, 1, 28, 28, generator=g)).numpy()[:, 0]


# ---- geometry cases ---------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (3, 5), (28, 28), (64, 64))
CELLS_PER_FRAME = (1, 2, 5, 6, 9)
NROWS = (1, 3, 8)
PADDINGS = (0, 1, 2)
N_FRAMES = (1, 3)
PAD_VALUES = (0.0, 0.5, 1.0)
N_IMAGES = 4                                      # fewer images than cells: one image fills several cells


def geometry_cases():
    """[(cells_per_frame, nrow, padding, n_frames, pad_value, rounding)], run for every image shape: the full product of the four
    tables; the pad value and the quantiser mode cycle through it"""
    out = []
    for i, (per_frame, nrow, padding, n_frames) in enumerate(itertools.product(CELLS_PER_FRAME, NROWS, PADDINGS, N_FRAMES)):
        out.append((per_frame, nrow, padding, n_frames, PAD_VALUES[i % 3], bool((i // 3) % 2)))
    return out


def determined_images(shape, rounding, seed):
    """(fp32 values (N_IMAGES, h, w), their bytes): 255 v = b + 0.5 (truncating) or 255 v + 0.5 = b + 0.5 (rounding) up to fp32
    rounding, i.e. half a step from the quantiser's edges: every byte is determined"""
    rs = np.random.RandomState(seed)
    b = rs.randint(0, 256, (N_IMAGES,) + tuple(shape))
    if not rounding:
        b = np.minimum(b, 254)                    # (255.5 / 255 would clamp all the same; keep the value inside [0, 1])
    v = ((b + (0.0 if rounding else 0.5)) / 255.0).astype(np.float32)
    return v, b.astype(np.uint8)


def geometry_cells(per_frame, n_frames, seed):
    """indices in [-1, N_IMAGES): blanks and repeats"""
    return np.random.RandomState(seed).randint(-1, N_IMAGES, (n_frames, per_frame))
