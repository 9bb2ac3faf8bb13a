"""CPU statement of the contrastive pre-training input (pixcontrast_18/contrast/data/dataset.py:43-70, transform.py:20-87,
transform_coord.py:81-224) with Pillow and numpy: the reference of stswincl_amd.contrast.views.ContrastViews.

Per view: `Image.fromarray(frame).crop((j, i, j + w, i + h)).resize((W, H), Image.BILINEAR)` for each of its four frames (what
F.resized_crop does), the same with NEAREST for its label, the flips, then ToTensor + Normalize as the fp32 table.  It works image by
image through Pillow itself, where the device works from per-view tap tables: the two share no code."""
from __future__ import annotations

import types

import numpy as np
import torch
from PIL import Image

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# dataset.py:56-68 written out: view k <- transform[k](...), stacked by append_img_1; frames 0 image, 1-4 prev1-prev4, 5-8 neg1 p1 p2
# p3, 9-12 the second negative's, 13-16 the third's
FRAME_MAP = ((3, 2, 1, 0), (3, 2, 1, 0), (4, 3, 2, 1), (8, 7, 6, 5), (12, 11, 10, 9), (16, 15, 14, 13))
LABEL_MAP = (0, 1, 2, 3, 4, 5)


def P(i, j, h, w, hflip=False, vflip=False):
    return types.SimpleNamespace(i=i, j=j, h=h, w=w, hflip=hflip, vflip=vflip)


def value_table(mean=MEAN, std=STD) -> np.ndarray:
    """fp32 [3][256]: ToTensor (`.to(float32).div(255)`) then Normalize (`.sub_(mean).div_(std)`, fp32 tensors), with torch CPU ops."""
    u = torch.arange(256, dtype=torch.uint8).to(dtype=torch.float32).div(255)
    planes = []
    for c in range(3):
        planes.append(u.clone().sub_(torch.tensor(mean[c], dtype=torch.float32)).div_(torch.tensor(std[c], dtype=torch.float32)))
    return torch.stack(planes).numpy()


def resized_crop(a: np.ndarray, p, out_hw, resample) -> np.ndarray:
    """uint8 [Hs][Ws] or [Hs][Ws][3] -> the same with (H, W): crop, resize, flips."""
    H, W = out_hw
    im = Image.fromarray(a).crop((p.j, p.i, p.j + p.w, p.i + p.h)).resize((W, H), resample)
    a = np.array(im)
    if p.hflip:
        a = a[:, ::-1]
    if p.vflip:
        a = a[::-1]
    return np.ascontiguousarray(a)


def view(frames4: np.ndarray, label: np.ndarray, p, out_hw, table: np.ndarray):
    """uint8 frames [4][Hs][Ws][3], label [Hs][Ws] -> (fp32 [4][3][H][W], fp32 [1][H][W])."""
    imgs = []
    for f in frames4:
        a = resized_crop(f, p, out_hw, Image.BILINEAR)
        imgs.append(np.stack([table[c][a[..., c]] for c in range(3)]))
    mask = resized_crop(label, p, out_hw, Image.NEAREST).astype(np.float32)[None]
    return np.stack(imgs), mask


def views(frames: np.ndarray, labels: np.ndarray, params, out_hw, frame_map=FRAME_MAP, label_map=LABEL_MAP, table=None):
    """uint8 frames [B][NF][Hs][Ws][3], labels [B][NL][Hs][Ws], params[b][v] -> (im_1 .. im_V, mask_1 .. mask_V) as torch CPU tensors:
    images fp32 [B][4][3][H][W], masks fp32 [B][1][H][W]."""
    table = value_table() if table is None else table
    ims, masks = [], []
    for v, (fm, lm) in enumerate(zip(frame_map, label_map)):
        res = [view(frames[b][list(fm)], labels[b][lm], params[b][v], out_hw, table) for b in range(len(params))]
        ims.append(torch.from_numpy(np.stack([r[0] for r in res])))
        masks.append(torch.from_numpy(np.stack([r[1] for r in res])))
    return tuple(ims) + tuple(masks)


def seeded_sample(seed: int, n_frames: int, n_labels: int, H: int, W: int, label_max: int = 255):
    """uint8 frames [n_frames][H][W][3] (gradients plus noise: neighbouring pixels and frames differ) and labels [n_labels][H][W]
    (blocks of 4 x 4 with values in 0 .. label_max, two corner pixels at 0 and label_max) that a test can regenerate from the seed."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    frames = np.empty((n_frames, H, W, 3), np.uint8)
    for t in range(n_frames):
        for c in range(3):
            base = (x * (3 + c) + y * (5 - c) + 37 * t + 60 * c) % 256
            frames[t, :, :, c] = (base + rng.integers(0, 48, (H, W))) % 256
    labels = rng.integers(0, label_max + 1, (n_labels, (H + 3) // 4, (W + 3) // 4), dtype=np.uint8).repeat(4, 1).repeat(4, 2)[:, :H, :W]
    labels = np.ascontiguousarray(labels)
    labels[:, 0, 0], labels[:, -1, -1] = 0, label_max                                  # both ends of the range are present
    return frames, labels
