"""Figure files of the image models: the bytes ops.render_frames produced on the device, written as PNG / GIF with PIL.

The reference goes through torchvision's save_image and utils/plotting.py:377-383 (save_gif_from_list); here the grid and the
cast to bytes are already done by the render launch, so a figure costs one device-to-host copy of its uint8 frames.
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


def write_gif(frames_u8, path, delay=100):
    """(F, H, W, C) frames as a looping GIF, `delay` ms per frame: the call of the reference's save_gif_from_list"""
    a = _host_u8(frames_u8)
    if a.ndim != 4 or a.shape[0] == 0:
        raise ValueError(f'a GIF takes (F, H, W, C) frames, got {a.shape}')
    images = [_image(f) for f in a]
    images[0].save(path, save_all=True, append_images=images[1:], optimize=False, duration=delay, loop=0)
    return path
