"""hip.bilinear, hip.logits_upsample, hip.rows_broadcast and hip.maxpool3x3s2 refuse operands that do not fit each other or the
stated geometry with StswinHipError BEFORE any launch: the checks read tensor attributes only, so most of them are tested here with
CPU tensors (no kernel can run on those at all); the device mismatch needs one tensor on the GPU.  Every test matches the message
of the check it is about, so that a later check (or the "tensors must be on the GPU" of the pointer conversion) cannot pass for it."""
import pytest
import torch

from stswincl_amd import hip

BF, F32 = torch.bfloat16, torch.float32
E = hip.StswinHipError


def _t(rows, cols, dt=F32, device="cpu"):
    return torch.zeros(rows, cols, dtype=dt, device=device)


# ------------------------------------------------------------------------------------------------------------------ bilinear
def test_bilinear_refuses_mixed_dtypes():
    with pytest.raises(E, match="source is torch.float32 but destination is torch.bfloat16"):
        hip.bilinear(_t(2 * 3, 8), _t(4 * 6, 8, BF), 1, 2, 3, 4, 6)
    with pytest.raises(E, match="source is torch.bfloat16 but destination is torch.float32"):
        hip.bilinear(_t(4 * 6, 8, BF), _t(2 * 3, 8), 1, 2, 3, 4, 6, backward=True)


def test_bilinear_refuses_unequal_widths():
    with pytest.raises(E, match="equally wide"):
        hip.bilinear(_t(6, 8), _t(24, 16), 1, 2, 3, 4, 6)


@pytest.mark.parametrize("src_rows,dst_rows,backward,what", [(5, 24, False, "src has 5 rows"), (6, 23, False, "dst has 23 rows"),
                                                             (6, 24, True, "src has 6 rows"), (24, 7, True, "dst has 7 rows"),
                                                             (12, 48, False, "src has 12 rows")])       # (two frames' rows, one stated)
def test_bilinear_refuses_rows_that_do_not_match_the_geometry(src_rows, dst_rows, backward, what):
    with pytest.raises(E, match=what):
        hip.bilinear(_t(src_rows, 8), _t(dst_rows, 8), 1, 2, 3, 4, 6, backward=backward)


# ------------------------------------------------------------------------------------------------------------------ logits_upsample
def test_logits_upsample_refuses_mixed_dtypes():
    with pytest.raises(E, match="tokens are torch.bfloat16 but the NCHW tensor is torch.float32"):
        hip.logits_upsample(_t(6, 64, BF), torch.zeros(1, 12, 16, 24), 1, 2, 3, 16, 24, 12)


def test_logits_upsample_refuses_a_token_matrix_narrower_than_the_classes():
    with pytest.raises(E, match="cannot hold 12 classes"):
        hip.logits_upsample(_t(6, 8), torch.zeros(1, 12, 16, 24), 1, 2, 3, 16, 24, 12)


def test_logits_upsample_refuses_rows_and_planes_that_do_not_match_the_geometry():
    with pytest.raises(E, match="tokens has 7 rows"):
        hip.logits_upsample(_t(7, 64), torch.zeros(1, 12, 16, 24), 1, 2, 3, 16, 24, 12)
    with pytest.raises(E, match="is not a contiguous"):
        hip.logits_upsample(_t(6, 64), torch.zeros(1, 12, 16, 23), 1, 2, 3, 16, 24, 12)
    with pytest.raises(E, match="is not a contiguous"):
        hip.logits_upsample(_t(6, 64), torch.zeros(1, 16, 24, 12).permute(0, 3, 1, 2), 1, 2, 3, 16, 24, 12, backward=True)


# ------------------------------------------------------------------------------------------------------------------ rows_broadcast
def test_rows_broadcast_refuses_a_v_that_is_not_contiguous_fp32():
    with pytest.raises(E, match="contiguous fp32"):
        hip.rows_broadcast(_t(3, 8, BF), _t(30, 8, BF), 3)
    with pytest.raises(E, match="contiguous fp32"):
        hip.rows_broadcast(_t(3, 16)[:, :8], _t(30, 8), 3)
    with pytest.raises(E, match="contiguous fp32"):
        hip.rows_broadcast(_t(8, 3).t(), _t(30, 8), 3)


def test_rows_broadcast_refuses_a_width_other_than_the_destination_s():
    with pytest.raises(E, match="equally wide"):
        hip.rows_broadcast(_t(3, 8), _t(30, 64), 3)
    with pytest.raises(E, match="equally wide"):
        hip.rows_broadcast(_t(3, 64), _t(30, 8, BF), 3)


@pytest.mark.parametrize("vrows,groups,M", [(2, 3, None), (3, 3, 31), (3, 3, 29), (3, 0, None), (4, 4, None)])
def test_rows_broadcast_refuses_rows_that_do_not_match_the_groups(vrows, groups, M):
    with pytest.raises(E, match="rows for"):
        hip.rows_broadcast(_t(vrows, 8), _t(30, 8), groups, M=M)


# ------------------------------------------------------------------------------------------------------------------ maxpool3x3s2
def _arg(rows, cols, device="cpu"):
    return torch.zeros(rows, cols, dtype=torch.uint8, device=device)


def test_maxpool_refuses_mixed_dtypes_and_widths():
    with pytest.raises(E, match="source is torch.float32 but destination is torch.bfloat16"):
        hip.maxpool3x3s2(_t(5 * 7, 8), _t(3 * 4, 8, BF), _arg(12, 8), 1, 5, 7, 3, 4)
    with pytest.raises(E, match="equally wide"):
        hip.maxpool3x3s2(_t(5 * 7, 8), _t(3 * 4, 16), _arg(12, 8), 1, 5, 7, 3, 4)


def test_maxpool_refuses_a_geometry_that_is_not_the_pool_s():
    with pytest.raises(E, match="is not the 3x3 stride-2 pad-1 pool"):
        hip.maxpool3x3s2(_t(5 * 7, 8), _t(2 * 3, 8), _arg(6, 8), 1, 5, 7, 2, 3)


@pytest.mark.parametrize("src_rows,dst_rows,backward,what", [(34, 12, False, "src has 34 rows"), (35, 13, False, "dst has 13 rows"),
                                                             (35, 12, True, "src has 35 rows"), (12, 36, True, "dst has 36 rows")])
def test_maxpool_refuses_rows_that_do_not_match_the_geometry(src_rows, dst_rows, backward, what):
    with pytest.raises(E, match=what):
        hip.maxpool3x3s2(_t(src_rows, 8), _t(dst_rows, 8), _arg(12, 8), 1, 5, 7, 3, 4, backward=backward)


def test_maxpool_refuses_an_arg_of_another_form():
    for arg in (_arg(11, 8), _arg(12, 16)[:, :8], torch.zeros(12, 8, dtype=torch.int32)):
        with pytest.raises(E, match="arg must be a contiguous uint8"):
            hip.maxpool3x3s2(_t(35, 8), _t(12, 8), arg, 1, 5, 7, 3, 4)


# ------------------------------------------------------------------------------------------------------------------ devices
@pytest.mark.gpu
def test_operands_on_different_devices_are_refused():
    """One operand on the GPU, the other on the CPU; the well-formed GPU destination is filled with a sentinel that must survive."""
    dst = torch.full((24, 8), 7.0, device="cuda")
    with pytest.raises(E, match="source on cpu but destination on cuda"):
        hip.bilinear(_t(6, 8), dst, 1, 2, 3, 4, 6)
    with pytest.raises(E, match="v on cpu but out on cuda"):
        hip.rows_broadcast(_t(3, 8), dst, 3)
    with pytest.raises(E, match="source on cpu but destination on cuda"):
        hip.maxpool3x3s2(_t(7 * 11, 8), dst, _arg(24, 8, "cuda"), 1, 7, 11, 4, 6)
    with pytest.raises(E, match="arg must be a contiguous uint8"):
        hip.maxpool3x3s2(_t(7 * 11, 8, device="cuda"), dst, _arg(24, 8), 1, 7, 11, 4, 6)
    nchw = torch.full((1, 8, 4, 6), 7.0, device="cuda")
    with pytest.raises(E, match="tokens on cpu but the NCHW tensor on cuda"):
        hip.logits_upsample(_t(6, 8), nchw, 1, 2, 3, 4, 6, 8)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((nchw == 7.0).all())


@pytest.mark.gpu
def test_mismatches_between_gpu_tensors_are_refused_and_nothing_is_written():
    dst = torch.full((24, 8), 7.0, dtype=BF, device="cuda")
    with pytest.raises(E, match="source is torch.float32 but destination is torch.bfloat16"):
        hip.bilinear(_t(6, 8, device="cuda"), dst, 1, 2, 3, 4, 6)
    with pytest.raises(E, match="equally wide"):
        hip.rows_broadcast(_t(3, 16, device="cuda"), dst, 3)
    with pytest.raises(E, match="contiguous fp32"):
        hip.rows_broadcast(_t(3, 8, BF, device="cuda"), dst, 3)
    with pytest.raises(E, match="dst has 24 rows"):
        hip.maxpool3x3s2(_t(2 * 7 * 11, 8, BF, device="cuda"), dst, _arg(48, 8, "cuda"), 2, 7, 11, 4, 6)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())
