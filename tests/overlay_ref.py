"""The numpy statement of stswin_labels_overlay (include/stswin_hip.h): blend, edge rule, NULL frames.  Integer arithmetic in int64."""
import numpy as np


def edges(labels: np.ndarray) -> np.ndarray:
    """bool [n][H][W]: the pixel's label differs from that of a left / right / upper / lower neighbour inside its own frame."""
    lab = np.asarray(labels)
    e = np.zeros(lab.shape, dtype=bool)
    d = lab[:, :, 1:] != lab[:, :, :-1]
    e[:, :, 1:] |= d
    e[:, :, :-1] |= d
    d = lab[:, 1:, :] != lab[:, :-1, :]
    e[:, 1:, :] |= d
    e[:, :-1, :] |= d
    return e


def overlay(labels: np.ndarray, table: np.ndarray, frames=None, edge_alpha=None) -> np.ndarray:
    """labels uint8 [n][H][W], table uint8 [256][4], frames uint8 [n][H][W][3] or None (all 0), edge_alpha None / -1 or 0 .. 255
    -> uint8 [n][H][W][3] = (a c + (255 - a) s + 127) // 255."""
    lab = np.asarray(labels)
    assert lab.dtype == np.uint8 and lab.ndim == 3 and table.dtype == np.uint8 and table.shape == (256, 4)
    entry = table[lab].astype(np.int64)                       # [n][H][W][4]
    c, a = entry[..., :3], entry[..., 3]
    if edge_alpha is not None and edge_alpha >= 0:
        a = np.where(edges(lab), edge_alpha, a)
    s = np.zeros(lab.shape + (3,), dtype=np.int64) if frames is None else np.asarray(frames).astype(np.int64)
    assert s.shape == lab.shape + (3,)
    a = a[..., None]
    return ((a * c + (255 - a) * s + 127) // 255).astype(np.uint8)
