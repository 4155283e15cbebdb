"""CPU: Program.plan, the workspace plan that the oracle and the device share (so a mistake in it cancels out of every parity test).  The
shipped programs, lowered with SynthWeights at one small size and at an operating size, and the one-layer programs of
tests/conv_cases.py that carry a split-K or an F(4x4) row-split scratch view:

  * every planned buffer lies inside workspace_floats at a 64-float boundary;
  * two buffers whose [first, last] op ranges intersect never overlap in address (`keep` = live to the end);
  * alias views (reshape, crop_rows) sit at their parent's offset and inside it;
  * every tensor an op touches -- a conv's scratch view included -- is live at that op."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as C  # noqa: E402
import sam_cases  # noqa: E402

from cartoonsegmentation_amd import nets  # noqa: E402
from cartoonsegmentation_amd import program as P  # noqa: E402
from cartoonsegmentation_amd.weights import SynthWeights  # noqa: E402

ALIGN = 64
END = 10 ** 9


def _floats(b):
    return b.n * b.h * b.w * b.c


def _root(b):
    while b.alias is not None:
        b = b.alias
    return b


def check_plan(prog):
    """-> (planned buffers, alias views, conv scratch views) after asserting the four properties"""
    top = prog.plan()
    assert top == prog.workspace_floats
    real = [b for b in prog.bufs if b.ext < 0 and b.alias is None and b.first is not None]
    for b in real:
        assert b.offset is not None and b.offset >= 0 and b.offset % ALIGN == 0 and b.offset + _floats(b) <= top, (prog.name, b.offset, _floats(b), top)
        assert b.first <= b.last
    # address overlap only between buffers that are never live together: sweep in address order
    iv = sorted((b.offset, b.offset + _floats(b), b.first, END if b.keep else b.last) for b in real)
    for i, (lo, hi, first, last) in enumerate(iv):
        for lo2, hi2, first2, last2 in iv[i + 1:]:
            if lo2 >= hi:
                break
            assert first2 > last or first > last2, "%s: [%d, %d) live over ops %d..%d and [%d, %d) live over ops %d..%d share addresses" % (
                prog.name, lo, hi, first, last, lo2, hi2, first2, last2)
    aliases = [b for b in prog.bufs if b.alias is not None]
    for b in aliases:
        r = _root(b)
        assert r.ext < 0 and b.offset == r.offset and _floats(b) <= _floats(r), (prog.name, b.offset, r.offset)
    # liveness: whatever an op reads or writes -- through an alias too -- belongs to a buffer that is planned and live at that op
    scratch = 0
    for i, o in enumerate(prog.ops):
        ids = [o['in0'], o['in1'], o['out'], o['scratch']]
        if o['scratch'] >= 0:
            assert o['kind'] == P.OP_CONV
            scratch += 1
        for t in ids:
            if t < 0:
                continue
            r = _root(prog.views[t].buf)
            if r.ext >= 0:
                continue
            assert r.first is not None and r.first <= i <= (END if r.keep else r.last), (prog.name, i, t, r.first, r.last)
    return len(real), len(aliases), scratch


def _prog(r):
    return r[0].prog if isinstance(r, tuple) else r


def _zoe(H, W):
    return nets.build_zoe_head(SynthWeights('zoe.'), 1, H, W, [(H >> s, W >> s) for s in (5, 4, 3, 2, 1)])


DPT_KW = dict(embed=64, depth=4, heads=2, base_grid=(4, 4), hooks=(0, 1, 2, 3), features=32, neck=(32, 32, 64, 64))
RTM_TINY = dict(deepen_factor=0.167, widen_factor=0.375, feat_channels=96)
SHIPPED = {
    'isnet-64': lambda: nets.build_isnet(SynthWeights('isnet.'), 1, 64, 64),
    'isnet-2x1024': lambda: nets.build_isnet(SynthWeights('isnet.'), 2, 1024, 1024),
    'isnet-128': lambda: nets.build_isnet(SynthWeights('isnet.'), 1, 128, 128),
    'leres-64x96': lambda: nets.build_leres(SynthWeights('leres.'), 1, 64, 96),
    'leres-2x448': lambda: nets.build_leres(SynthWeights('leres.'), 2, 448, 448),
    'rtmdet-l-64': lambda: nets.build_rtmdet(SynthWeights('rtmdet.'), 1, 64, 64),
    'rtmdet-l-2x640': lambda: nets.build_rtmdet(SynthWeights('rtmdet.'), 2, 640, 640),
    'rtmdet-tiny-96': lambda: nets.build_rtmdet(SynthWeights('rtmdet.'), 1, 96, 96, nets.RTMDetConfig(**RTM_TINY)),
    'rtmdet-tiny-640': lambda: nets.build_rtmdet(SynthWeights('rtmdet.'), 1, 640, 640, nets.RTMDetConfig(**RTM_TINY)),
    'refine-50x70': lambda: nets.build_refine(SynthWeights('refine.'), 50, 70, 25, 35),
    'refine-1024x768': lambda: nets.build_refine(SynthWeights('refine.'), 1024, 768, 512, 384),
    'inpaint-context-32x48': lambda: nets.build_inpaint_context(SynthWeights('inpaint.'), 32, 48),
    'inpaint-context-768x1024': lambda: nets.build_inpaint_context(SynthWeights('inpaint.'), 768, 1024),
    'inpaint-grid-33x47': lambda: nets.build_inpaint_grid(SynthWeights('inpaint.'), 33, 47),       # an odd size: the GridNet's cropped adds
    'inpaint-grid-96x128': lambda: nets.build_inpaint_grid(SynthWeights('inpaint.'), 96, 128),
    'inpaint-grid-768x1024': lambda: nets.build_inpaint_grid(SynthWeights('inpaint.'), 768, 1024),
    'semantics-64x96': lambda: nets.build_semantics(SynthWeights('semantics.'), 64, 96),
    'semantics-512x384': lambda: nets.build_semantics(SynthWeights('semantics.'), 512, 384),
    'disparity-64x96': lambda: nets.build_disparity(SynthWeights('disparity.'), 64, 96),
    'disparity-512x384': lambda: nets.build_disparity(SynthWeights('disparity.'), 512, 384),
    'dpt-beit-64x96': lambda: nets.build_dpt_beit(SynthWeights('dpt.'), 2, 64, 96, nets.DPTBeitConfig(**DPT_KW)),
    'dpt-beit-256x384': lambda: nets.build_dpt_beit(SynthWeights('dpt.'), 1, 256, 384, nets.DPTBeitConfig(**DPT_KW)),
    'zoe-head-64x96': lambda: _zoe(64, 96),
    'zoe-head-384x512': lambda: _zoe(384, 512),
    'sam-encoder-a': lambda: nets.build_sam_encoder(SynthWeights('sam.'), nets.SamConfig(**sam_cases.CFG_A), 1),
    'sam-encoder-b': lambda: nets.build_sam_encoder(SynthWeights('sam.'), nets.SamConfig(**sam_cases.CFG_B), 1),
    'sam-decoder-a-1': lambda: nets.build_sam_decoder(SynthWeights('sam.'), nets.SamConfig(**sam_cases.CFG_A), 1),
    'sam-decoder-b-3': lambda: nets.build_sam_decoder(SynthWeights('sam.'), nets.SamConfig(**sam_cases.CFG_B), 3),
}


@pytest.mark.parametrize("name", list(SHIPPED))
def test_shipped_program_plans_without_overlap(name):
    prog = _prog(SHIPPED[name]())
    nb, na, ns = check_plan(prog)
    print("%s: %d ops, %d planned buffers, %d alias views, %d conv scratch views, %d floats" % (name, len(prog.ops), nb, na, ns, prog.workspace_floats))
    assert nb >= 3
    if name == 'isnet-128':
        assert nb == 243
    if name == 'inpaint-grid-96x128':
        assert nb == 134


def test_alias_views_and_scratch_views_are_really_exercised():
    """the properties about aliases and scratch are not vacuous: the SAM decoder reshapes its token buffer, the small nets split K and
    plan the F(4x4) row-split scratch"""
    got = {name: check_plan(_prog(SHIPPED[name]())) for name in ('sam-decoder-a-1', 'rtmdet-tiny-96', 'zoe-head-64x96')}
    assert got['sam-decoder-a-1'][1] > 0 and got['rtmdet-tiny-96'][2] > 0 and got['zoe-head-64x96'][2] > 0


def test_row_crop_and_reshape_views_keep_their_parent_alive():
    """no shipped net uses crop_rows today: a program whose cropped and reshaped views are read long after the last direct use of their
    parents, with buffers born and freed in between"""
    p = P.Program('aliases')
    x_ext, y_ext = p.ext_nchw(1, 8, 6, 5), p.ext_nchw(1, 8, 4, 5)
    x = p.to_nhwc(x_ext)
    a = p.act(x, 'relu')
    top = p.crop_rows(a, 4)                                                # a's first four rows
    flat = p.reshape(p.act(x, 'silu'), 1, 1, 1, 6 * 5 * 8)                 # another buffer as one pixel of 240 channels
    t = x
    for _ in range(4):                                                     # buffers that come and go while `a` and `flat`'s parent only wait
        t = p.act(t, 'relu')
    s = p.add(top, p.crop_rows(t, 4))
    p.to_nchw(s, y_ext)
    p.copy(flat.slice(0, 8), p.buffer(1, 1, 1, 16).slice(8, 16))
    nb, na, _ = check_plan(p)
    assert na == 3 and nb >= 6
    last = len(p.ops) - 1
    assert a.buf.last == [i for i, o in enumerate(p.ops) if o['in0'] == top.id][0] and flat.buf.alias.last == last
    for b in p.bufs:
        if b.alias is not None:
            assert b.offset == b.alias.offset


def test_one_layer_programs_with_split_k_or_row_split_scratch():
    n = 0
    for k in C.splitk_cases() + C.f4_cases() + [k for k in C.epilogue_cases() if k['cls'] in ('splitk', 'f4')]:
        b = C.program(k)
        if b.aux is None:
            continue
        nb, _, ns = check_plan(b.prog)
        assert ns == 1
        op = C.conv_op(b)
        need = op['ksplit'] * k['w'].shape[0] if op['ksplit'] > 1 else 24 * k['w'].shape[0]
        assert b.aux.c == need and b.aux.buf.first == b.aux.buf.last == b.prog.ops.index(op), k['name']
        n += 1
    assert n >= len(C.splitk_cases()) + 10
