"""CPU-side checks of the C-ABI boundary: the library builds, loads, and exports every declared symbol;
the product path has no CPU fallback (it must fail loudly)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import __graft_entry__ as ge
from stswincl_amd import hip


def test_library_builds_and_exports_declared_abi():
    ge.build(verbose=False)
    lib = hip.load()
    syms = hip.declared_symbols()
    assert len(syms) >= 12 and "stswin_gemm_nt" in syms and "stswin_win_attn_bwd" in syms
    for s in syms:
        assert hasattr(lib, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(syms) <= exported
    assert lib.stswin_abi_version() == 1


def _header_text():
    with open(hip.HEADER_PATH) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_argtypes_follow_the_header_prototypes():
    """Every declared entry point carries the argtypes of its prototype: as many as the prototype has parameters, long -> c_long,
    float -> c_float, double -> c_double, int -> c_int, anything with a `*` -> c_void_p; a few signatures are pinned by hand so that the
    test is not only the parser agreeing with itself."""
    ge.build(verbose=False)
    lib = hip.load()
    text = _header_text()
    scalar = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
    seen = 0
    for s in hip.declared_symbols():
        m = re.search(r"\b(int|long)\s+" + s + r"\s*\(([^()]*)\)\s*;", text)
        assert m, s
        params = [] if m.group(2).strip() == "void" else [p.strip() for p in m.group(2).split(",")]
        fn = getattr(lib, s)
        assert fn.restype is scalar[m.group(1)], s
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (s, params)
        for p, t in zip(params, fn.argtypes):
            want = ctypes.c_void_p if "*" in p else scalar[p.replace("const ", "").split()[0]]
            assert t is want, (s, p, t)
        seen += len(params)
    assert len(hip.declared_symbols()) >= 93 and seen >= 1000
    nt = lib.stswin_gemm_nt.argtypes
    assert len(nt) == 24 and all(nt[i] is ctypes.c_long for i in (2, 5, 7, 10, 13)) and nt[19] is ctypes.c_float
    assert nt[0] is ctypes.c_int and nt[1] is ctypes.c_void_p and nt[23] is ctypes.c_void_p
    assert [i for i, t in enumerate(nt) if t is ctypes.c_long] == [2, 5, 7, 10, 13]
    ce = lib.stswin_ce_fwd.argtypes                      # (dtype, logits, labels, loss, stats, frames, HW, nc, ignore_index, thresh, stream)
    assert len(ce) == 11 and ce[6] is ctypes.c_long and ce[9] is ctypes.c_float
    assert lib.stswin_abi_version.argtypes == []
    tick = lib.stswin_optim_tick.argtypes
    assert tick[3] is ctypes.c_double and tick[4] is ctypes.c_double
    assert lib.stswin_calib_mfma.restype is ctypes.c_long and lib.stswin_stem_wgrad_scratch.restype is ctypes.c_long


def test_wrong_argument_count_or_type_is_refused_before_the_call():
    """ctypes checks the arguments against argtypes before anything reaches the library (nothing is launched here)."""
    ge.build(verbose=False)
    lib = hip.load()
    with pytest.raises(TypeError):
        lib.stswin_ce_fwd(0, None, None, None, None, 1, 1 << 33, 8, 255, 0.7)                  # the stream is missing
    with pytest.raises(TypeError):
        lib.stswin_gemm_nt(0, None, 64)
    with pytest.raises(ctypes.ArgumentError):
        lib.stswin_ce_fwd(0, None, None, None, None, 1, 1024.0, 8, 255, 0.7, None)             # a float where HW (long) is declared
    with pytest.raises(ctypes.ArgumentError):
        lib.stswin_gemm_nt_splitk_scratch(4096, 512, 1024.5, 9)                                # ... and where an int is
    with pytest.raises(ctypes.ArgumentError):
        lib.stswin_stem_wgrad(None, None, None, 0, None, "many", 1, 256, 256, None)


def test_header_parser_refuses_what_it_does_not_know(tmp_path, monkeypatch):
    """An unrecognised parameter or #define value raises, naming the function / the macro: never an int by default."""
    for body, culprit in (("int stswin_bad(int n, size_t bytes, void* stream);", "stswin_bad"),
                          ("int stswin_bad2(unsigned flags);", "stswin_bad2"),
                          ("float stswin_bad3(int n);", "stswin_bad3"),
                          ("int stswin_bad4(int (*callback)(int), void* stream);", "stswin_bad4"),
                          ("#define STSWIN_BAD_VALUE (sizeof(int) * 2)\nint stswin_ok(void);", "STSWIN_BAD_VALUE"),
                          ("#define STSWIN_BAD_DIV (8 / 2)\nint stswin_ok(void);", "STSWIN_BAD_DIV")):
        h = tmp_path / "bad.h"
        h.write_text("/* c */\n" + body + "\n")
        monkeypatch.setattr(hip, "HEADER_PATH", str(h))
        hip._header.cache_clear()
        try:
            with pytest.raises(hip.StswinHipError, match=culprit):
                hip._header()
        finally:
            monkeypatch.undo()
            hip._header.cache_clear()
    assert "stswin_gemm_nt" in hip.declared_symbols()


# what tests/, tools/, bench.py and the package's own modules use today, with the values they had as hand-typed copies
_PINNED = dict(
    GF_GELU=1, GF_RESID=2, GF_MUL_DGELU=4, GF_OUT_F32=8, GF_ACCUM=16, GF_RELU=32, GF_WAVES4=64, GF_BIG=128, GF_NOBIG=256, GF_MID=512,
    GF_NOPIPE=1024, GF_HALF=2048, GF_ROT=4096, GF_MUL_R=8192, GF_C2_DGELU=16384, GF_CS_PARTIAL=32768, GF_CS_SQ=1 << 16,
    GF_NOREGEPI=1 << 22, GF_NOSTREAM=1 << 23, GF_DUO=1 << 24, GF_STREAM=1 << 25, GF_NONARROW=1 << 26, GF_NODEEP=1 << 27, GF_DEEP=1 << 28,
    GF_TAPSKIP=1 << 29, GF_W4R=1 << 30, GF_M32PP=-(1 << 31), TN_OVERWRITE=1 << 27, TN_NO_COMBINE=1 << 26, TN_OUT_TAPMINOR=1 << 25,
    TN_GROUP_DECLINED=-1050, OHEM_WORK_BYTES=3 * 2048 * 12 + 48, VAR_F32=100, VAR_NT_RING256_REGEPI=1, VAR_NT_RING256_LDSEPI=2,
    VAR_NT_RING256_NOPIPE=3, VAR_NT_STREAM=4, VAR_NT_DUO=5, VAR_NT_RING256x128_PP=6, VAR_NT_MID=7, VAR_NT_256x64=8, VAR_NT_128x64=9,
    VAR_NT_128x128=10, VAR_NT_128x128_W4=11, VAR_NT_ROWS=12, VAR_NT_SPLITK=13, VAR_NT_RING256_W4=14, VAR_TN_RING_PLAIN=20,
    VAR_TN_RING_ATROWS=21, VAR_TN_RING_BTROWS=22, VAR_TN_RING_BSEG=23, VAR_TN_128x128=30, VAR_TN_128x128_W4=31, VAR_TN_ROWS=32,
    VAR_TN_SLABS_F32=0x1000, VAR_TN_SLABS_BF16=0x2000, VAR_TN_TAPMINOR=0x4000, VAR_TN_FUSED=0x8000)


def test_constants_are_the_header_defines():
    """Every `#define STSWIN_X value` has its hip.X twin with the same value (bit 31 of a flags word is the sign bit of the C int it
    travels in), the names in use keep their values, and no GF_ / TN_ / VAR_ literal is typed into hip.py any more."""
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+STSWIN_(\w+)[ \t]+(\S.*)$", _header_text(), flags=re.M)
    assert len(defines) >= 58
    for name, expr in defines:
        assert re.fullmatch(r"[0-9a-fA-Fx\s()<*+\-]+", expr.replace("u", "")), (name, expr)
        want = eval(expr.replace("u", ""))                                    # (integer literals and operators only: checked above)
        assert hasattr(hip, name), name
        assert (getattr(hip, name) - want) % (1 << 32) == 0 and -(1 << 31) <= getattr(hip, name) < 1 << 31, (name, expr)
    assert {n for n, _ in defines} == set(_PINNED)
    for name, value in _PINNED.items():
        assert getattr(hip, name) == value, name
    for name in ("tn_fused_holds", "_Span", "profile_begin", "profile_step", "profile_end", "calibrate", "load", "arena_reset",
                 "_PROFILE_ALWAYS", "_p", "_stream", "_NT_SPLITK", "_CS_PARTIAL_MIN_M", "_TN_PENDING", "_tn_workspace", "scratch",
                 "declared_symbols", "StswinHipError", "LAST_TN_GROUP_SPLITS", "VARIANT_LOG"):
        assert hasattr(hip, name), name


def test_tn_problem_matches_the_header_struct():
    """hip._TnProblem is written by hand: its fields must be those of `typedef struct stswin_tn_problem`, in order and in type."""
    m = re.search(r"typedef\s+struct\s+stswin_tn_problem\s*\{(.*?)\}\s*stswin_tn_problem\s*;", _header_text(), flags=re.S)
    assert m
    scalar = {"int": ctypes.c_int, "long": ctypes.c_long}
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype = ctypes.c_void_p if "*" in decl else scalar[decl.split()[0]]
            head, *more = decl.split(",")                       # `int Mk, Ni, Nj, bseg`
            fields += [(n.replace("*", " ").split()[-1], ctype) for n in [head] + more]
    assert fields == list(hip._TnProblem._fields_)
    assert len(fields) == 14


def test_no_hand_marshalling_left_in_the_package():
    """Source-level guard: with argtypes in place no call site wraps an argument in a ctypes object, and hip.py assigns no GF_ / TN_ /
    VAR_ constant of its own."""
    pkg = os.path.dirname(hip.__file__)
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(root, f)) as fh:
                    src = fh.read()
                for bad in re.findall(r"\b_c_long\(|\b_c_float\(|c_void_p\(|\bc_long\(|\bc_float\(|\bc_double\(", src):
                    raise AssertionError(f"{f}: `{bad}` wraps an argument by hand")
    with open(hip.__file__) as fh:
        src = fh.read()
    assert not re.findall(r"^\s*(?:[\w, ()]*\b(?:GF|TN|VAR)_[A-Z]\w*[\w, ()]*|OHEM_WORK_BYTES|_OHEM_WORK_BYTES)\s*=[^=]", src, flags=re.M)
    assert not hasattr(hip, "_cs_table") and not hasattr(hip, "_CS_TABLES") and not hasattr(hip, "_c_long")


def test_code_object_targets_gfx950_only():
    out = subprocess.run(["strings", "-n", "6", hip.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    for other in ("gfx90a", "gfx942", "sm_80"):
        assert other not in out


def test_no_cpu_fallback():
    x = torch.zeros(8, 64)
    with pytest.raises(hip.StswinHipError):
        hip.layernorm_fwd(x, torch.ones(64), torch.zeros(64), M=8)


def test_dataparallel_replica_threads_are_refused_loudly():
    """seg18/train_swin.py:131-135 wraps the model in nn.DataParallel.  Over several GPUs that means replica threads inside one
    process, which the per-process caches of this package do not support: a replica must raise with the one-process-per-GPU
    recipe instead of racing (a single-device DataParallel calls the module itself and is unaffected)."""
    from stswincl_amd.net.Ours.base18 import TswinPlus
    m = TswinPlus(12, (8, 8))
    m._is_replica = True                       # what torch.nn.parallel.replicate sets on every replica module
    with pytest.raises(hip.StswinHipError, match="one\\s+process per GPU"):
        m(torch.zeros(1, 4, 3, 64, 64))
