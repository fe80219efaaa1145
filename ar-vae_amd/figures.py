"""Figure files of the image models: the bytes ops.render_frames produced on the device, written as PNG / GIF with PIL.

The reference goes through torchvision's save_image and utils/plotting.py:377-383 (save_gif_from_list); here the grid and the
cast to bytes are already done by the render launch, so a figure costs one device-to-host copy of its uint8 frames.
The piano rolls (ops.render_pianoroll) and the scatter figures of the latent plane (ops.render_scatter; write_data_dist is both
trainers' plot_data_dist) are written the same way.
"""
import numpy as np
import torch


def _host_u8(frames):
    """uint8 frames as a host array (one copy when they live on the device)"""
    a = frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    if a.dtype != np.uint8:
        raise TypeError(f'figure frames are uint8 (ops.render_frames), got {a.dtype}')
    return a


def _image(frame):
    """(H, W, 3) -> RGB, (H, W, 1) or (H, W) -> greyscale"""
    from PIL import Image
    if frame.ndim == 3 and frame.shape[2] == 1:
        frame = frame[:, :, 0]
    if not (frame.ndim == 2 or (frame.ndim == 3 and frame.shape[2] == 3)):
        raise ValueError(f'a frame is (H, W, 3), (H, W, 1) or (H, W), got {frame.shape}')
    return Image.fromarray(np.ascontiguousarray(frame))


def write_png(frame_u8, path):
    """one frame, (H, W, C) or (1, H, W, C), as a PNG file"""
    a = _host_u8(frame_u8)
    if a.ndim == 4 and a.shape[0] == 1:
        a = a[0]
    _image(a).save(path)
    return path


def write_data_dist(trainer, latent_codes, attributes, names, columns, dim1, dim2, look):
    """data_dist_{name}.png for every name (both trainers' plot_data_dist; the reference's plot_dim with xlim = ylim = 4,
    utils/plotting.py:41-63): figure i shows the codes in the plane (dim1[i], dim2[i]) coloured by column columns[i] of
    `attributes`.  dim1 / dim2: one dimension for all figures or one each.  All figures of a call (16 at most a launch) are
    rendered by one ops.render_scatter launch and reach the host in one copy.  -> the paths written"""
    import os
    from . import ops
    from .trainer import Trainer
    codes = np.asarray(latent_codes.detach().cpu() if torch.is_tensor(latent_codes) else latent_codes, dtype=np.float32)
    attrs = np.asarray(attributes.detach().cpu() if torch.is_tensor(attributes) else attributes, dtype=np.float32)
    if codes.ndim != 2 or attrs.ndim != 2 or codes.shape[0] != attrs.shape[0]:
        raise ValueError(f'plot_data_dist takes codes (n, z_dim) and attributes (n, k), got {codes.shape} and {attrs.shape}')
    f = len(names)
    dims = [[int(d)] * f if np.ndim(d) == 0 else [int(x) for x in d] for d in (dim1, dim2)]
    if len(dims[0]) != f or len(dims[1]) != f:
        raise ValueError(f'plot_data_dist: dim1 and dim2 are one dimension or {f} of them')
    dev = next(trainer.model.parameters()).device
    folder = Trainer.get_save_dir(trainer.model)
    paths = []
    for at in range(0, f, 16):
        part = range(at, min(at + 16, f))
        points = torch.from_numpy(np.stack([codes[:, [dims[0][i], dims[1][i]]] for i in part])).to(dev)
        values = torch.from_numpy(np.stack([attrs[:, columns[i]] for i in part])).to(dev)
        labels = [(f'dimension: {dims[0][i]}', f'dimension: {dims[1][i]}') for i in part]
        frames = ops.render_scatter(points.contiguous(), values.contiguous(), (-4.0, 4.0), (-4.0, 4.0), **{'labels': labels, **look}).cpu().numpy()
        paths += [write_png(frames[k], os.path.join(folder, f'data_dist_{names[i]}.png')) for k, i in enumerate(part)]
    return paths


def write_gif(frames_u8, path, delay=100):
    """(F, H, W, C) frames as a looping GIF, `delay` ms per frame: the call of the reference's save_gif_from_list"""
    a = _host_u8(frames_u8)
    if a.ndim != 4 or a.shape[0] == 0:
        raise ValueError(f'a GIF takes (F, H, W, C) frames, got {a.shape}')
    images = [_image(f) for f in a]
    images[0].save(path, save_all=True, append_images=images[1:], optimize=False, duration=delay, loop=0)
    return path
