"""CPU: the table of conv tile configurations (csrc/csm_convcfg.h + the rows of the kernel family files) against the list it replaced,
the autotuner's candidate order, and the fall-back rules of the executor (resolve_cfg).  Host code only: no device is touched."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (id, name, family, BN) -- transcribed from the enum, the launch switch and the tuner's arrays this table replaced.
# BN: MT * WN * TN for k_conv_mfma, 32 * TN * WN for the LDS-DMA / patch kernels, 32 * TN for k_conv_ws, 4 for k_conv_narrow.
EXPECTED = [
    (0, "128x128_4w", "MFMA", 128), (1, "128x64", "MFMA", 64), (2, "64x64", "MFMA", 64), (3, "128x128_8w", "MFMA", 128),
    (4, "128x32", "MFMA", 32), (5, "64x16", "MFMA", 16),
    (6, "D64x64", "DMA", 64), (7, "D128x64", "DMA", 64), (8, "D128x128", "DMA", 128), (9, "D128x128_8w", "DMA", 128),
    (10, "D256x128_8w", "DMA", 128), (11, "D64x128", "DMA", 128), (12, "D128x32", "DMA", 32),
    (13, "NARROW", "NARROW", 4),
    (14, "D96x128", "DMA", 128), (15, "D160x128", "DMA", 128), (16, "D224x128", "DMA", 128), (17, "D192x128", "DMA", 128),
    (18, "P64x64", "PATCH", 64), (19, "P128x64", "PATCH", 64), (20, "P64x128", "PATCH", 128), (21, "P128x128", "PATCH", 128),
    (22, "P256x128", "PATCH", 128), (23, "P128x32", "PATCH", 32), (24, "P64x64_w8", "PATCH", 64), (25, "P128x128_w8", "PATCH", 128),
    (26, "P128x32_w8", "PATCH", 32), (27, "P128x128_8w", "PATCH", 128),
    (28, "D64x64_s3", "DMA", 64), (29, "D128x64_s3", "DMA", 64), (30, "D64x128_s3", "DMA", 128), (31, "D128x128_s3", "DMA", 128),
    (32, "D128x128_8w_s3", "DMA", 128), (33, "D256x128_8w_s3", "DMA", 128), (34, "D256x64", "DMA", 64), (35, "D256x64_s3", "DMA", 64),
    (36, "P256x64", "PATCH", 64), (37, "D64x64_s4", "DMA", 64),
    (38, "Q64x64", "DMA_P", 64), (39, "Q128x64", "DMA_P", 64), (40, "Q64x128", "DMA_P", 128), (41, "Q128x128_8w", "DMA_P", 128),
    (42, "Q128x32", "DMA_P", 32),
    (43, "R128x32", "PATCH_P", 32), (44, "R64x64", "PATCH_P", 64), (45, "R128x64", "PATCH_P", 64), (46, "R128x32_w8", "PATCH_P", 32),
    (47, "R128x128_8w", "PATCH_P", 128), (48, "R64x128", "PATCH_P", 128), (49, "R64x64_w8", "PATCH_P", 64),
    (50, "R128x128_8w_o4", "PATCH_P", 128),
    (51, "W256x32", "WS", 32), (52, "W256x64", "WS", 64),
]
TUNE_ORDER = [2, 4, 5, 6, 7, 11, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 38, 39, 40, 41, 42,
              43, 44, 45, 47, 48, 50, 51, 52]


@pytest.fixture(scope="module")
def lib():
    lib_path = os.path.join(ROOT, "cartoonsegmentation_amd", "libcsm355.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    from cartoonsegmentation_amd import _lib
    return _lib.load()


def test_table_matches_the_list_it_replaced(lib):
    from cartoonsegmentation_amd.runtime import conv_cfg_table
    assert lib.csm_debug_conv_cfg_count() == 53
    table = conv_cfg_table()
    assert [(c['id'], c['name'], c['family'], c['bn']) for c in table] == EXPECTED
    assert [c['id'] for c in table] == list(range(53))


def test_tuner_order_is_unchanged(lib):
    from cartoonsegmentation_amd.runtime import conv_cfg_table
    assert len(TUNE_ORDER) == 38
    timed = sorted((c['tune_pos'], c['id']) for c in conv_cfg_table() if c['tune_pos'] >= 0)
    assert [pos for pos, _ in timed] == list(range(38))
    assert [cid for _, cid in timed] == TUNE_ORDER


def test_id_outside_the_table_is_an_error(lib):
    from cartoonsegmentation_amd.runtime import _ConvCfgDesc
    d = _ConvCfgDesc()
    for cfg in (-1, 53, 64):
        assert lib.csm_debug_conv_cfg_info(ctypes.c_int(cfg), ctypes.byref(d)) != 0
    assert lib.csm_debug_conv_cfg_info(ctypes.c_int(52), ctypes.byref(d)) == 0


ID = {name: cid for cid, name, _, _ in EXPECTED}

# (k, dil, cin, cout, groups, cfg in, id out): h = w = 40, stride 1, pad = dil * (k // 2); every tensor 16-byte aligned, ld % 4 == 0.
# Expected ids follow the four rules by hand:
#  1. WS that is not patch-eligible or does not fit 160 KB of LDS (86 016 B of patch stages + 9 * ncb * BN * 128 B of weights) -> R64x64
#  2. PATCH / PATCH_P / WS on a layer that is not a 3x3 stride 1 dilation 1 DMA-eligible one -> D64x64
#  3. NARROW with cout > 4 -> 64x16
#  4. any LDS-DMA family with cin_g % 32 != 0 -> 64x16 / 128x32 / 64x64 by cout_g <= 16 / <= 32 / more
RESOLVE_CASES = [
    (3, 1, 64, 96, 1, "W256x32", 51),      # 86 016 + 73 728 B fit
    (3, 1, 64, 96, 1, "W256x64", 44),      # 86 016 + 147 456 B do not: rule 1, and R64x64 can run it
    (1, 1, 32, 96, 1, "W256x64", 6),       # 1x1: rule 1 then rule 2
    (1, 1, 32, 96, 1, "R64x64", 6),        # rule 2
    (1, 1, 32, 96, 1, "Q64x64", 38),       # the persistent DMA kernel runs a 1x1
    (3, 4, 256, 256, 1, "P64x64", 6),      # dilated: rule 2
    (3, 1, 16, 96, 1, "R64x64", 2),        # cin_g 16: rule 2 then rule 4
    (3, 1, 16, 24, 1, "R64x64", 4),
    (3, 1, 16, 8, 1, "R64x64", 5),
    (3, 1, 64, 8, 1, "NARROW", 5),         # rule 3
]


@pytest.mark.parametrize("case", RESOLVE_CASES, ids=["%s-k%dd%d-%dto%d" % (c[5], c[0], c[1], c[2], c[3]) for c in RESOLVE_CASES])
def test_resolve_cfg(lib, case):
    from cartoonsegmentation_amd.program import OP_CONV, CsmOp, CsmTensorDesc
    k, dil, cin, cout, groups, name, want = case
    n, h, w = 1, 40, 40
    op = CsmOp(kind=OP_CONV, in0=0, in1=-1, out=1, kh=k, kw=k, stride=1, pad=dil * (k // 2), dil=dil, groups=groups, cin_g=cin // groups,
               cout_g=cout // groups, act=0, res_mode=0, w_off=0, b_off=-1, aux_off=-1, flags=0, ksplit=1, scratch=-1, tile=0)
    tin = CsmTensorDesc(0, -1, n, h, w, cin, cin)
    tout = CsmTensorDesc(n * h * w * cin, -1, n, h, w, cout, cout)
    assert (n * h * w * cin) % 4 == 0 and cin % 4 == 0 and cout % 4 == 0
    got = lib.csm_debug_conv_resolve_cfg(ctypes.c_int(ID[name]), ctypes.byref(op), ctypes.byref(tin), ctypes.byref(tout))
    assert got == want
