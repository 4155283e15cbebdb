"""CPU: the GIF contract as tests/gif_restatement.py states it -- Pillow decodes every file to palette[indices], the
restatement's own decoder returns the indices, the cases reach every width a Clear and an EOI can be written at -- and the host
product code of the route: gifcode.build_palette, the container and its error paths."""
import functools
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gif_restatement as R  # noqa: E402

S = R.S
SIZES = [S - 1, S, S + 1, 2 * S + 5]
NOREPEAT = [254, 255, 256, 257, 1000, S, S + 255, S + 256, S + 1000, 2 * S + 5]         # 1000: an EOI at 11 bits
# flat frames whose streams end in a sub-block of 255 bytes and of 1 byte (found by search over the restatement)
FLAT_255, FLAT_1 = 28359, 38496
CASES = (['one', 'rect-67x131', 'flat-61x67', 'mask-50x91', 'noise-50x91', 'flat-1x%d' % FLAT_255, 'flat-1x%d' % FLAT_1]
         + ['noise-1x%d' % n for n in SIZES] + ['noise-%dx1' % n for n in SIZES]
         + ['norepeat-%d' % n for n in NOREPEAT])


def _norepeat():
    """a, b for every a < b with a ascending: 65 280 indices in which no adjacent pair occurs twice"""
    a, b = np.triu_indices(256, 1)
    return np.stack([a, b], axis=1).reshape(-1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def indices(name, variant=0):
    """the index frame of a case, uint8 [H,W]; variants 1 and 2 are other frames of the same shape (for stacked clips)"""
    kind, _, size = name.partition('-')
    rng = np.random.default_rng([sum(name.encode()), variant])
    if kind == 'one':
        a = np.array([[7 + variant]], np.uint8)
    elif kind == 'norepeat':
        a = _norepeat()[:int(size)][None, :]
        a = a if variant == 0 else (a + variant).astype(np.uint8)            # adding a constant keeps the pairs distinct
    else:
        H, W = (int(v) for v in size.split('x'))
        if kind == 'flat':
            a = np.full((H, W), 200 + variant, np.uint8)
        elif kind == 'mask':
            a = np.where(rng.random((H, W)) < 0.5, 3, 250).astype(np.uint8)
        elif kind == 'rect':
            yy, xx = np.mgrid[0:H, 0:W]
            a = ((yy // 3 + xx // 5 + rng.integers(0, 2, (H, W))) % 17 * 15).astype(np.uint8)
        else:
            assert kind == 'noise', name
            a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(name, variant=0):
    """(LZW bytes, trace) of the restatement"""
    trace = {}
    return R.lzw(indices(name, variant), trace), trace


# a fixed palette with distinct entries, so a decoded colour names its index
PALETTE = np.stack([np.arange(256), (np.arange(256) * 7 + 3) % 256, 255 - np.arange(256)], axis=1).astype(np.uint8)


def pil_frames(data):
    """(frames as RGB arrays, durations, loop) of a GIF file through Pillow"""
    im = Image.open(io.BytesIO(data))
    assert im.format == 'GIF'
    frames, durations = [], []
    for k in range(im.n_frames):
        im.seek(k)
        durations.append(im.info.get('duration'))
        frames.append(np.asarray(im.convert('RGB')))
    return frames, durations, im.info.get('loop')


def check_gif(data, index_frames, palette, order=None):
    """Pillow reads the frames `order` names, each exactly palette[indices], 40 ms apiece; the loop count is there unless the file
    has one frame"""
    order = list(range(len(index_frames))) if order is None else order
    frames, durations, loop = pil_frames(data)
    assert len(frames) == len(order)
    for got, i in zip(frames, order):
        assert np.array_equal(got, palette[index_frames[i]])
    assert (loop == 0) if len(order) > 1 else (loop is None)
    if len(order) > 1:
        assert durations == [40] * len(order)


@pytest.mark.parametrize("name", CASES)
def test_restatement_decodes_in_pillow_and_in_its_own_decoder(name):
    a = indices(name)
    stream = want(name)[0]
    assert len(stream) <= R.bound(*a.shape)
    assert np.array_equal(R.unlzw(stream, a.size).reshape(a.shape), a)
    data = R.gif([stream], a.shape[1], a.shape[0], PALETTE)
    check_gif(data, [a], PALETTE)
    clip = [indices(name, v) for v in range(3)]
    streams = [want(name, v)[0] for v in range(3)]
    data = R.gif(streams, a.shape[1], a.shape[0], PALETTE)
    assert data == R.encode_indices(np.stack(clip), PALETTE)
    check_gif(data, clip, PALETTE)


def test_cases_cover_every_width_and_both_sub_block_ends():
    clears, eois, lasts, equal = set(), set(), set(), False
    for name in CASES:
        tr = want(name)[1]
        clears |= tr['clear_widths']
        eois |= tr['eoi_widths']
        lasts |= tr['last_entries']
        equal |= tr['code_equals_next']
    assert clears == {9, 10, 11, 12} and eois == {9, 10, 11, 12}
    assert 4095 in lasts and equal
    assert len(want('flat-1x%d' % FLAT_255)[0]) % 255 == 0 and len(want('flat-1x%d' % FLAT_1)[0]) % 255 == 1
    for name in ('flat-1x%d' % FLAT_255, 'flat-1x%d' % FLAT_1):
        blocks = R.frame_blocks(want(name)[0])
        sizes, pos = [], 0
        while blocks[pos]:
            sizes.append(blocks[pos])
            pos += 1 + blocks[pos]
        assert pos == len(blocks) - 1 and sizes[-1] == (255 if name.endswith(str(FLAT_255)) else 1) and set(sizes[:-1]) <= {255}


def test_playback_order_file_and_the_product_container():
    """2n - 2 frames in ping-pong order; gifcode.gif_file (the product's container) writes the restatement's bytes"""
    from cartoonsegmentation_amd import gifcode, video
    clip = [indices('rect-67x131', v) for v in range(4)]
    streams = [R.lzw(f) for f in clip]
    order = video.playback_order(4)
    assert order == [0, 1, 2, 3, 2, 1]
    data = R.gif(streams, 131, 67, PALETTE, order=order)
    check_gif(data, clip, PALETTE, order)
    assert gifcode.gif_file(streams, 131, 67, PALETTE, fps=25, loop=0, order=order) == data
    assert gifcode.gif_file(streams[:1], 131, 67, PALETTE) == R.gif(streams[:1], 131, 67, PALETTE)
    assert gifcode.gif_file(streams, 131, 67, PALETTE, fps=10, loop=3) == R.gif(streams, 131, 67, PALETTE, fps=10, loop=3)
    for name in ('flat-1x%d' % FLAT_255, 'flat-1x%d' % FLAT_1, 'one', 'noise-1x%d' % S):
        assert gifcode.sub_blocks(want(name)[0]) == R.frame_blocks(want(name)[0])
    assert gifcode.stream_bound(67, 131) == R.bound(67, 131) and gifcode.SEGMENT == S
    assert np.array_equal(gifcode.BAYER, R.BAYER)


def test_write_gif_writes_the_file(tmp_path):
    from cartoonsegmentation_amd import video
    clip = [indices('rect-67x131', v) for v in range(3)]
    streams = [want('rect-67x131', v)[0] for v in range(3)]
    path = str(tmp_path / "a.gif")
    size = video.write_gif(path, streams, 131, 67, PALETTE, order=[0, 1, 2, 1])
    data = open(path, 'rb').read()
    assert size == len(data) and data == R.gif(streams, 131, 67, PALETTE, order=[0, 1, 2, 1])
    check_gif(data, clip, PALETTE, [0, 1, 2, 1])


# ---- the palette --------------------------------------------------------------------------------------------------------------
def colour_frames(name):
    """BGR test clips by name: 'noise' 2 x 17x23 of random colours, 'five' 2 x 40x56 of 5 colours, 'few' 3 x 31x45 of 200 colours that
    fall into 200 different cells, 'smooth' 2 x 64x64 gradients"""
    rng = np.random.default_rng(sum(name.encode()))
    if name == 'noise':
        return rng.integers(0, 256, (2, 17, 23, 3), dtype=np.uint8)
    if name == 'five':
        cols = np.array([[0, 0, 0], [255, 255, 255], [13, 200, 77], [14, 90, 201], [250, 3, 128]], np.uint8)
        return cols[rng.integers(0, 5, (2, 40, 56))]
    if name == 'few':
        cells = rng.choice(32768, 200, replace=False)
        cols = np.stack([cells >> 10, (cells >> 5) & 31, cells & 31], axis=1) * 8 + rng.integers(0, 8, (200, 3))
        return cols.astype(np.uint8)[rng.integers(0, 200, (3, 31, 45))]
    assert name == 'smooth'
    yy, xx = np.mgrid[0:64, 0:64]
    a = np.stack([yy * 4, xx * 4, (yy + xx) * 2], axis=2).astype(np.uint8)
    return np.stack([a, a[::-1, :, ::-1]])


def test_build_palette_is_deterministic_and_bounded():
    from cartoonsegmentation_amd import gifcode
    for name in ('noise', 'smooth', 'five'):
        table = R.cell_table(colour_frames(name))
        assert int(table[:, 0].sum()) == colour_frames(name)[..., 0].size
        p = gifcode.build_palette(table)
        assert p.dtype == np.uint8 and p.shape == (256, 3)
        assert p.tobytes() == gifcode.build_palette(table.copy()).tobytes()
    # 782 occupied cells of the noise clip: all 256 entries are used, and every entry lies inside the colour range of its box
    p = gifcode.build_palette(R.cell_table(colour_frames('noise')))
    assert len({tuple(e) for e in p}) > 200
    assert gifcode.build_palette(np.zeros((32768, 4), np.uint32)).tobytes() == bytes(768)
    with pytest.raises(ValueError):
        gifcode.build_palette(np.zeros((4096, 4), np.uint32))


def test_257_cells_merge_exactly_one_pair():
    """one cell more than the palette has entries: 255 cells keep their own colour, two share the mean of theirs"""
    from cartoonsegmentation_amd import gifcode
    table = np.zeros((32768, 4), np.uint32)
    keys = np.arange(257) * 101                                              # 257 occupied cells
    table[keys, 0] = 5
    table[keys[7], 0] = 1                                                    # the lightest cell
    p = gifcode.build_palette(table)
    cols = np.stack([keys >> 10, (keys >> 5) & 31, keys & 31], axis=1) * 8
    hit = [(cols[i] == p).all(axis=1).any() for i in range(257)]
    assert sum(hit) >= 255                                                   # every cell but one merged pair keeps its own colour
    assert len({tuple(e) for e in p}) == 256


@pytest.mark.parametrize("name", ['five', 'few'])
def test_a_clip_of_at_most_256_single_colour_cells_is_lossless(name):
    from cartoonsegmentation_amd import gifcode
    frames = colour_frames(name)
    p = gifcode.build_palette(R.cell_table(frames))
    colours = {tuple(int(v) for v in c[::-1]) for c in frames.reshape(-1, 3)}
    used = [tuple(int(v) for v in e) for e in p[:len(colours)]]
    assert set(used) == colours and not p[len(colours):].any()
    for dither in ('none', 'ordered'):
        idx = R.quantize(frames, p, dither)
        assert np.array_equal(p[idx], frames[..., ::-1])
        data = R.encode_indices(idx, p)
        got = pil_frames(data)[0]
        assert all(np.array_equal(g, f[..., ::-1]) for g, f in zip(got, frames))


def test_mapping_takes_the_lower_of_duplicate_entries_and_dithers_by_position_only():
    p = PALETTE.copy()
    p[200] = p[10]
    p[11] = p[10]
    frames = np.broadcast_to(p[10][::-1], (1, 9, 9, 3)).copy()
    frames[0, 4, 4] = (p[10][::-1].astype(int) + [1, 0, 0]).astype(np.uint8)  # one off: still nearest to the duplicates
    for dither in ('none', 'ordered'):
        idx = R.quantize(frames, p, dither)
        assert idx[0, 0, 0] == 10 and (idx != 200).all() and (idx != 11).all()
    # the dither depends on (y & 7, x & 7) only: shifting a flat off-palette frame by 8 changes nothing, and every frame of a clip
    # gets the same pattern
    grey = np.stack([np.arange(256)] * 3, axis=1).astype(np.uint8)[::8]      # 32 greys, 8 apart
    pal = np.zeros((256, 3), np.uint8)
    pal[:32] = grey
    flat = np.full((2, 24, 24, 3), 100, np.uint8)                            # between the entries 96 and 104
    idx = R.quantize(flat, pal, 'ordered')
    assert set(np.unique(idx)) == {12, 13}
    assert np.array_equal(idx[0], idx[1]) and np.array_equal(idx[0, 8:, 8:], idx[0, :16, :16])
    assert (R.quantize(flat, pal, 'none') == 12).all()                       # 100 is nearer to 96; at equal distance the lower index


# ---- error paths --------------------------------------------------------------------------------------------------------------
def test_error_paths():
    torch = pytest.importorskip("torch")
    from cartoonsegmentation_amd import gifcode, ops
    from cartoonsegmentation_amd._lib import CsmError
    ok = [want('one')[0]]
    for w, h in ((0, 1), (1, 0), (65536, 1), (1, 65536)):
        with pytest.raises(ValueError):
            gifcode.gif_file(ok, w, h, PALETTE)
    for fps in (0, -1, 201, 1e-4, float('nan')):                             # a delay of 0 cs (fps above 200), or above 65535
        with pytest.raises(ValueError):
            gifcode.gif_file(ok, 1, 1, PALETTE, fps=fps)
        with pytest.raises(ValueError):
            ops.gif_encode(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), fps=fps)
    assert gifcode.delay_cs(25) == 4 and gifcode.delay_cs(200) == 1 and gifcode.delay_cs(30) == 3 and gifcode.delay_cs(40) == 3
    for order in ([1], [-1], [0, 2], []):
        with pytest.raises(ValueError):
            gifcode.gif_file(ok, 1, 1, PALETTE, order=order)
    with pytest.raises(ValueError):
        gifcode.gif_file(ok, 1, 1, PALETTE[:255])
    with pytest.raises(ValueError):
        gifcode.gif_file(ok, 1, 1, PALETTE.astype(np.int32))
    for bad in (torch.zeros((4, 4, 3)), torch.zeros((2, 4, 4, 4), dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8),
                torch.zeros((1, 2, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 4, 4, 3), dtype=torch.bool), np.zeros((4, 4), np.uint8)):
        with pytest.raises(CsmError):
            ops.gif_quantize(bad)
        with pytest.raises(CsmError):
            ops.gif_encode(bad)
    for bad in (torch.zeros((4, 4), dtype=torch.int32), torch.zeros((1, 2, 4, 4), dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.bool)):
        with pytest.raises(CsmError):
            ops.gif_streams(bad)
    for shape in ((0, 4), (4, 0), (1, 65536), (65536, 1), (2, 0, 4)):
        with pytest.raises(ValueError):
            ops.gif_streams(torch.zeros(shape, dtype=torch.uint8))
        with pytest.raises(ValueError):
            ops.gif_quantize(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(CsmError):
        ops.gif_streams(torch.zeros((4, 4), dtype=torch.uint8))              # a CPU tensor: libcsm355 has no CPU path
    with pytest.raises(ValueError):
        ops.gif_quantize(torch.zeros((4, 4, 3), dtype=torch.uint8), dither='floyd')
    with pytest.raises(ValueError):
        ops.gif_quantize(torch.zeros((4, 4, 3), dtype=torch.uint8), palette=PALETTE[:16])
