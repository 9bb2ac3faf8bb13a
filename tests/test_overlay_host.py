"""Host side of the colour overlay (CPU): stswincl_amd/utils/visualize.py against the recorded output of the reference's
segcata/utils/cadis_visualization.py (tests/golden/overlay_colormap.npz, tools/gen_golden_overlay.py) and against tests/overlay_ref.py,
the numpy statement of the kernel."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import overlay_ref as O
from stswincl_amd import hip
from stswincl_amd.utils import visualize as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay_colormap.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _colormap(golden, k):
    return {int(key): tuple(int(v) for v in color) for key, color in zip(golden[f"exp{k}/keys"], golden[f"exp{k}/colors"])}


def test_the_fixture_is_what_the_generator_documents(golden):
    mask = golden["mask"]
    assert mask.dtype == np.uint8 and mask.shape == (24, 40)
    assert set(np.unique(mask).tolist()) == set(range(36)) | {255}
    for k, classes in ((1, 8), (2, 17), (3, 25)):
        keys = golden[f"exp{k}/keys"].tolist()
        assert keys[:classes] == list(range(classes)) and set(keys) <= set(range(classes)) | {255}
        assert golden[f"exp{k}/colors"].shape == (len(keys), 3) and golden[f"exp{k}/rgb"].shape == (24, 40, 3)
        assert 255 in np.unique(golden[f"exp{k}/remapped"])


@pytest.mark.parametrize("k", [1, 2, 3])
def test_opaque_overlay_without_edges_is_mask_to_colormap_and_the_recorded_picture(golden, k):
    remapped, want = golden[f"exp{k}/remapped"], golden[f"exp{k}/rgb"]
    cmap = _colormap(golden, k)
    host = V.mask_to_colormap(remapped, cmap)
    assert host.dtype == np.uint8 and np.array_equal(host, want)
    table = V.overlay_table(cmap, alpha=255)
    rng = np.random.default_rng(k)
    frame = rng.integers(0, 256, (1,) + remapped.shape + (3,), dtype=np.uint8)
    for frames in (None, frame):                           # alpha 255 hides the frame, except where the colormap has no key
        got = O.overlay(remapped[None], table, frames)[0]
        keyed = np.isin(remapped, list(cmap))
        assert np.array_equal(got[keyed], want[keyed])
        if frames is None:
            assert np.array_equal(got, want)               # (black where no key matches, as the reference)
        else:
            assert np.array_equal(got[~keyed], frame[0][~keyed])
    assert np.array_equal(O.overlay(remapped[None], table, frame, edge_alpha=-1), O.overlay(remapped[None], table, frame))


def test_mask_to_colormap_semantics():
    mask = np.array([[0, 1, 2], [7, 255, 1]], dtype=np.int64)
    cmap = {1: [10, 20, 30], 255: [0, 0, 0], 7: np.array([1, 2, 3])}
    got = V.mask_to_colormap(mask, cmap)
    want = np.zeros((2, 3, 3), np.uint8)
    want[0, 1] = want[1, 2] = (10, 20, 30)
    want[1, 0] = (1, 2, 3)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(V.mask_to_colormap(mask.astype(np.uint8), cmap), want)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_palette_from_colormap_round_trips_the_recorded_dict(golden, k):
    cmap = _colormap(golden, k)
    pal = V.palette_from_colormap(cmap)
    assert pal.dtype == np.uint8 and pal.shape == (max(cmap) + 1, 3)
    assert (255 in cmap) == (len(pal) == 256)
    for key, color in cmap.items():
        assert tuple(pal[key].tolist()) == color, key
    assert not pal[[i for i in range(len(pal)) if i not in cmap]].any()
    assert np.array_equal(V.palette_from_colormap(pal), pal)                        # the [n][3] array form
    assert np.array_equal(V.palette_from_colormap(pal.astype(np.int64).tolist()), pal)
    for bad in ({}, {256: (0, 0, 0)}, {1: (0, 0, 256)}, {1: (0, 0)}, np.zeros((4, 4)), np.zeros((257, 3))):
        with pytest.raises(ValueError):
            V.palette_from_colormap(bad)


def test_overlay_table_alphas_transparency_and_labels_beyond_the_palette():
    pal = np.arange(30, dtype=np.uint8).reshape(10, 3)
    t = V.overlay_table(pal)
    assert t.dtype == np.uint8 and t.shape == (256, 4)
    assert np.array_equal(t[:10, :3], pal) and (t[:10, 3] == 128).all() and not t[10:].any()
    t = V.overlay_table(pal, alpha=200, transparent=(0, 9, 40), alphas={3: 255, 9: 7})
    assert t[0, 3] == 0 and t[9, 3] == 7 and t[3, 3] == 255 and t[40, 3] == 0
    assert (t[[1, 2, 4, 5, 6, 7, 8], 3] == 200).all() and np.array_equal(t[:10, :3], pal) and not t[10:].any()
    full = V.overlay_table({0: (1, 2, 3), 255: (0, 0, 0)}, alpha=255, transparent=(255,))
    assert tuple(full[0]) == (1, 2, 3, 255) and tuple(full[255]) == (0, 0, 0, 0) and (full[1:255, 3] == 255).all()
    for kwargs in (dict(alpha=256), dict(alpha=-1), dict(alpha=1.5), dict(transparent=(256,)), dict(alphas={1: 300})):
        with pytest.raises(ValueError):
            V.overlay_table(pal, **kwargs)


def test_default_palette_follows_its_stated_formula():
    pal = V.default_palette()
    assert pal.dtype == np.uint8 and pal.shape == (256, 3)
    for i in range(256):
        want = [sum(((i >> (3 * j + ch)) & 1) << (7 - j) for j in range(3)) for ch in range(3)]
        assert pal[i].tolist() == want, i
    assert len({tuple(c) for c in pal.tolist()}) == 256 and not pal[0].any()
    assert pal[1].tolist() == [128, 0, 0] and pal[2].tolist() == [0, 128, 0] and pal[4].tolist() == [0, 0, 128] and pal[8].tolist() == [64, 0, 0]


def test_reference_statement_rounding_and_edges():
    """overlay_ref itself: exact ends of the blend, round-half-up in between, and the edge rule on a hand-made map."""
    table = np.zeros((256, 4), np.uint8)
    table[:, 0] = 200
    table[:, 3] = np.arange(256)
    lab = np.arange(256, dtype=np.uint8)[None, :, None].repeat(256, 2)
    fr = np.zeros((1, 256, 256, 3), np.uint8)
    fr[..., 0] = np.arange(256)[None, None, :]
    got = O.overlay(lab, table, fr)[0, :, :, 0].astype(np.float64)
    a, s = np.arange(256.)[:, None], np.arange(256.)[None, :]
    exact = (a * 200 + (255 - a) * s) / 255
    assert np.abs(got - exact).max() <= 0.5 and np.array_equal(got[255], np.full(256, 200.)) and np.array_equal(got[0], np.arange(256.))
    m = np.zeros((2, 4, 5), np.uint8)
    m[0, 1, 2] = 3
    m[1] = 9                                                  # another constant frame: no edge between frames
    e = O.edges(m)
    want = np.zeros((2, 4, 5), bool)
    want[0, 1, 1:4] = want[0, 0, 2] = want[0, 2, 2] = True
    assert np.array_equal(e, want)


def test_header_declares_the_entry_point_and_the_library_exports_it():
    assert "stswin_labels_overlay" in hip.declared_symbols()
    ge.build(verbose=False)
    lib = hip.load()
    fn = lib.stswin_labels_overlay
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    assert callable(hip.labels_overlay)
