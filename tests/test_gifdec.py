"""CPU: the contract of the GIF decoder.  The numpy restatement (tests/gifdec_restatement.py) equals Pillow on every
frame of every file of tests/gifdec_cases.py, for RGB and RGBA; the set of files has the properties it is there for;
gifread.probe reports the structure and refuses what it should; the host-only container parsers of video.read_avi and
video.read_apng return the frames that were written; and the code walker of the kernels (csrc/csm_lzw.h), built for the host under
the address and undefined-behaviour sanitizers as a program of its own, agrees on valid streams and stays inside its buffers on
truncated and mutated ones."""
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gifdec_cases as C  # noqa: E402
import gifdec_restatement as R  # noqa: E402
from cartoonsegmentation_amd import gifread, video  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def parsed():
    out = {}
    for name in C.NAMES:
        data = C.case_file(name)
        info = gifread.probe(data)
        stats = []
        out[name] = (info, R.decode_indices(data, info, stats), stats)
    return out


@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_equals_pillow(name, alpha, parsed):
    info, indices, _ = parsed[name]
    ref = C.reference(name, alpha)
    got = R.compose(info, indices, alpha)
    assert got.shape == ref.shape == (len(info['frames']), info['height'], info['width'], 4 if alpha else 3)
    assert got.dtype == np.uint8
    for k in range(len(ref)):
        wrong = int((got[k] != ref[k]).any(axis=-1).sum())
        assert wrong == 0, "%s frame %d: %d pixels differ from Pillow" % (name, k, wrong)
    assert [fr['duration'] for fr in info['frames']] == C.durations(name)


def test_the_set_has_its_lzw_properties(parsed):
    st = {name: C.STREAMS[name] for name in C.NAMES}
    for m in range(2, 9):
        info = parsed['mcs%d' % m][0]
        assert info['frames'][0]['min_code_size'] == m and (info['height'], info['width']) == (9, 13)
        assert parsed['mcs%d' % m][1][0].max() >= (1 << m) - 2              # the indices use the code size
    assert {(parsed[n][0]['height'], parsed[n][0]['width']) for n in ('size_1x1', 'size_1x7', 'size_5x1')} == {(1, 1), (1, 7), (5, 1)}
    full, defer, every = st['dict_clear'][0], st['dict_defer'][0], st['dict_every100'][0]
    assert full['codes'] > 4096 and full['max_next'] >= 4095 and full['clears'] >= 2        # a clear when the dictionary fills
    assert defer['codes'] > 4096 and defer['max_next'] == 4096 and defer['clears'] == 1      # full, and never cleared again
    assert every['clears'] >= 40 and every['max_next'] < 512
    flat = st['flat'][0]
    assert flat['self_ref'] >= 50 and flat['codes'] < 80                # nearly every code equals the next free entry
    assert parsed['flat'][2][0]['rounds'] >= 5 and max(s['rounds'] for n in C.NAMES for s in parsed[n][2]) >= 5
    assert st['no_first_clear'][0]['clears'] == 0
    blocks = parsed['blocks'][0]['frames'][0]
    assert blocks['stream_bytes'] % 4 != 0 and len(blocks['blocks']) >= 2 and blocks['blocks'][0][1] - blocks['blocks'][0][0] == 255
    assert len(parsed['small_blocks'][0]['frames'][0]['blocks']) > 10
    # junk behind the end code: the stream is longer than its codes
    data = C.case_file('junk')
    fr = parsed['junk'][0]['frames'][0]
    rec, err = R.walk(gifread.lzw_stream(data, fr), 4, 9 * 13)
    assert err == 0 and gifread.lzw_stream(data, fr).tobytes().endswith(b'\x5a\xa5\xff\x00\x13')
    for h in (1, 2, 3, 4, 5, 9):
        info = parsed['lace_h%d' % h][0]
        assert info['frames'][0]['interlace'] and info['height'] == h
    assert parsed['comment87'][0]['version'] == b'GIF87a' and not C.case_file('comment87').endswith(b';')


def test_the_set_has_its_animation_properties(parsed):
    H, W = C.CANVAS_H, C.CANVAS_W
    frames = lambda name: parsed[name][0]['frames']  # noqa: E731
    for name in C.NAMES:
        if name.startswith('anim_'):
            assert (parsed[name][0]['height'], parsed[name][0]['width']) == (H, W)
            assert all(fr['min_code_size'] == 4 for fr in frames(name))
    fr = frames('anim_rects')
    assert any(f['left'] + f['width'] == W and f['top'] + f['height'] < H for f in fr)
    assert any(f['top'] + f['height'] == H and f['left'] + f['width'] < W for f in fr)
    assert any((f['width'], f['height']) == (1, 1) for f in fr) and any(f['interlace'] for f in fr)
    for name, transparent in (('anim_disposal_t', True), ('anim_disposal_nt', False)):
        assert {f['disposal'] for f in frames(name)} == {0, 2, 3}
        assert all((f['transparent'] is not None) == transparent for f in frames(name))
        raw = [(b >> 2) & 7 for b in gce_flags(C.case_file(name))]
        assert set(raw) == {0, 1, 2, 3}                                  # all four methods stand in the file
    assert frames('anim_mixed_t')[0]['transparent'] is None and frames('anim_mixed_t')[1]['transparent'] is not None
    assert frames('anim_t0_only')[0]['transparent'] is not None and frames('anim_t0_only')[1]['transparent'] is None
    loc = frames('anim_local')
    assert [f['palette'] is not None for f in loc] == [False, True, True, True, False]
    short = [k for k, f in enumerate(loc) if f['palette'] is not None and parsed['anim_local'][1][k].max() >= len(f['palette']) // 3]
    assert short, "no local table shorter than the indices used"
    assert any(loc[k]['transparent'] is not None and loc[k]['transparent'] >= len(loc[k]['palette']) // 3 for k in short)
    assert parsed['anim_local0_short'][1][0].max() >= len(frames('anim_local0_short')[0]['palette']) // 3
    assert parsed['anim_no_global'][0]['global_palette'] is None
    for name in ('anim_small0', 'anim_small0_t'):
        f0 = frames(name)[0]
        assert f0['width'] < W and f0['height'] < H and f0['left'] > 0 and f0['top'] > 0
    assert frames('anim_prev0')[0]['disposal'] == 3 and frames('anim_prev0')[0]['transparent'] is None
    assert frames('anim_prev0_t')[0]['disposal'] == 3 and frames('anim_prev0_t')[0]['transparent'] is not None
    raw = [(b >> 2) & 7 for b in gce_flags(C.case_file('anim_sticky'))]
    assert raw == [2, 0, 0] and [f['disposal'] for f in frames('anim_sticky')] == [2, 2, 2, 2]   # the last frame has no extension
    assert parsed['anim_bg'][0]['background'] == 11 and parsed['anim_mixed_t'][0]['background'] == 6
    assert [f['duration'] for f in frames('anim_delay0')] == [0, 0, 655350] and parsed['anim_delay0'][0]['loop'] == 7
    assert parsed['gifcode'][0]['loop'] == 2 and len(frames('gifcode')) == 4
    assert len(frames('pillow_a')) == 3 and len(frames('pillow_b')) == 4
    # Pillow's writer: delta rectangles with a transparent index and local tables in one clip, whole frames disposed to background in the other
    assert any(f['width'] < parsed['pillow_a'][0]['width'] and f['transparent'] is not None and f['palette'] for f in frames('pillow_a'))
    assert all(f['disposal'] == 2 and f['width'] == parsed['pillow_b'][0]['width'] for f in frames('pillow_b'))


def gce_flags(data):
    """the flag bytes of the graphic control extensions of one of the writer's own files, in file order"""
    out, p = [], 0
    while True:
        p = data.find(b'\x21\xf9\x04', p)
        if p < 0:
            return out
        out.append(data[p + 3])
        p += 8


@pytest.mark.parametrize("name", C.NAMES)
def test_probe_fields(name, parsed):
    info = parsed[name][0]
    data = C.case_file(name)
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.size == (info['width'], info['height'])
        assert im.n_frames == len(info['frames'])
        assert im.info.get('loop') == info['loop']
        assert im.info.get('background', 0) == info['background']
    for k, fr in enumerate(info['frames']):
        assert 0 <= fr['left'] and fr['left'] + fr['width'] <= info['width'] and 0 <= fr['top'] and fr['top'] + fr['height'] <= info['height']
        assert fr['stream_bytes'] == sum(e - s for s, e in fr['blocks']) == gifread.lzw_stream(data, fr).size
        assert fr['disposal'] in (0, 2, 3)
        d = gifread.image_descriptor(fr, 3, 4096, 768, 16, 1 << 33)
        assert d.dtype == np.int32 and d.shape == (gifread.DESC_WORDS,) and (int(d[12]) | int(d[13]) << 31) == 1 << 33
        assert (d[0], d[1], d[2], d[3], d[14], d[15]) == (fr['height'], fr['width'], fr['top'], fr['left'], 3, 0)
    f = gifread.file_descriptor(info, 5, 1 << 34, 3)
    assert f.shape == (gifread.FILE_WORDS,) and (int(f[4]) | int(f[5]) << 31) == 1 << 34 and f[3] == len(info['frames'])
    assert f[7] == (1 if info['frames'][0]['transparent'] is not None else 0)


@pytest.mark.parametrize("name", sorted(C.REFUSED))
def test_probe_refuses_with_the_reason(name):
    build, word = C.REFUSED[name]
    with pytest.raises(gifread.Unsupported) as e:
        gifread.probe(build())
    assert word in str(e.value), str(e.value)


def test_probe_raises_nothing_else_on_prefixes_and_mutations():
    rng = np.random.default_rng(5)
    for name in ('anim_local', 'comment87', 'small_blocks'):
        data = C.case_file(name)
        for n in range(len(data)):
            try:
                gifread.probe(data[:n])
            except gifread.Unsupported:
                pass
        for _ in range(300):
            m = bytearray(data)
            m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
            try:
                gifread.probe(bytes(m))
            except gifread.Unsupported:
                pass


# ---- the container parsers of read_avi and read_apng ------------------------------------------------------------------------------
def test_avi_frames_returns_the_jpegs_written(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    jpegs = []
    for k in range(3):
        buf = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (20, 36, 3)).astype(np.uint8)).save(buf, 'JPEG', quality=80 + k)   # odd and even sizes
        jpegs.append(buf.getvalue())
    path = tmp_path / "clip.avi"
    video.write_mjpeg_avi(str(path), jpegs, 36, 20, fps=8, order=[0, 1, 2, 1])
    data = path.read_bytes()
    width, height, frames, ms = video.avi_frames(data)
    assert (width, height) == (36, 20) and frames == [jpegs[0], jpegs[1], jpegs[2], jpegs[1]] and ms == 125.0
    assert any(len(j) & 1 for j in jpegs), "no chunk with padding"
    for n in (0, 11, 200, len(data) - 1):
        with pytest.raises(video.Unsupported):
            video.avi_frames(data[:n])
    with pytest.raises(video.Unsupported, match="codec"):
        video.avi_frames(data.replace(b'MJPG', b'H264'))
    with pytest.raises(video.Unsupported, match="complete JPEG"):
        video.avi_frames(data.replace(jpegs[2], jpegs[2][:-2] + b'\x00\x00'))


def test_apng_frames_returns_files_pillow_decodes_to_the_frames(tmp_path):
    import zlib
    from PIL import Image
    rng = np.random.default_rng(4)
    for ct, shape in ((2, (3, 14, 9, 3)), (0, (2, 5, 7))):
        frames = rng.integers(0, 256, shape).astype(np.uint8)
        streams = [zlib.compress(b''.join(b'\x00' + row.tobytes() for row in f), 6) for f in frames]
        order = list(range(len(frames))) + [0]
        path = tmp_path / ("clip%d.apng" % ct)
        video.write_apng(str(path), streams, shape[2], shape[1], ct, fps=10, order=order)
        data = path.read_bytes()
        width, height, files, durations = video.apng_frames(data)
        assert (width, height) == (shape[2], shape[1]) and len(files) == len(order) and durations == [100.0] * len(order)
        with Image.open(io.BytesIO(data)) as im:
            assert im.n_frames == len(order)
            for k, f in enumerate(files):
                im.seek(k)
                with Image.open(io.BytesIO(f)) as one:
                    assert one.mode == im.mode and np.array_equal(np.asarray(one), np.asarray(im))
                    assert np.array_equal(np.asarray(one), frames[order[k]])
        for n in (0, 8, 40, len(data) - 1):
            with pytest.raises(video.Unsupported):
                video.apng_frames(data[:n])
    with Image.open(io.BytesIO(files[0])) as one:
        buf = io.BytesIO()
        one.save(buf, 'PNG')
    with pytest.raises(video.Unsupported, match="acTL"):
        video.apng_frames(buf.getvalue())


def test_read_video_refuses_other_suffixes():
    with pytest.raises(ValueError, match="mp4"):
        video.read_video("clip.mp4")


# ---- the walker of the kernels, on the host -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("walker") / "lzw_host_check"
    # the sanitizer runtimes are linked statically: the program then needs nothing of them at load time, whatever the environment
    # it inherits preloads
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
           "-I", os.path.join(ROOT, "cartoonsegmentation_amd", "csrc"), os.path.join(ROOT, "tools", "lzw_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run_walker(exe, tmp_path, streams, window=0, batch=0, indices=False):
    """[(error word, pixels, hash, indices or None)] of (pixels, minimum code size, LZW bytes) triples, one process for all of them;
    window: the bytes of the staging window the walker reads through (0: the whole stream); batch: records per step"""
    lines = []
    for k, (npix, mcs, s) in enumerate(streams):
        p = tmp_path / ("s%d.lzw" % k)
        p.write_bytes(s)
        lines.append("%d %d %s\n" % (npix, mcs, p))
    opts = (["-w", str(window)] if window else []) + (["-b", str(batch)] if batch else []) + (["-x"] if indices else [])
    r = subprocess.run([exe] + opts + ["-"], input="".join(lines), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(streams)
    return [(int(row[0]), int(row[1]), int(row[2], 16), bytes.fromhex(row[3]) if len(row) > 3 else (b'' if indices else None)) for row in rows]


def image_streams(name):
    data = C.case_file(name)
    info = gifread.probe(data)
    return [(fr['height'] * fr['width'], fr['min_code_size'], gifread.lzw_stream(data, fr).tobytes()) for fr in info['frames']]


def stream_order(ind, fr):
    return ind[C.lace_order(fr['height'])] if fr['interlace'] else ind


def test_walker_equals_the_restatement_on_every_case(walker, tmp_path, parsed):
    streams, want = [], []
    for name in C.NAMES:
        streams += image_streams(name)
        want += [stream_order(ind, fr).tobytes() for ind, fr in zip(parsed[name][1], parsed[name][0]['frames'])]
    for window, batch in ((0, 0), (16, 1), (1024, 64)):               # 1024 and 64 are the kernel's; 16 restages at every step
        got = run_walker(walker, tmp_path, streams, window, batch, indices=True)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g[0] == 0 and g[1] == len(w) and g[3] == w, (k, window, batch)


def test_walker_on_truncated_and_mutated_streams(walker, tmp_path):
    """every prefix of three streams and a few hundred seeded single-byte mutations: a clean exit with a non-zero error word or the
    right size, and no sanitizer report (run_walker asserts a clean stderr)"""
    rng = np.random.default_rng(11)
    streams = []
    for name in ('mcs2', 'lace_h9', 'flat'):
        npix, mcs, s = image_streams(name)[0]
        streams += [(npix, mcs, s[:k]) for k in range(len(s))]
    for name in ('mcs8', 'blocks', 'dict_defer', 'flat', 'anim_local', 'mcs3'):
        npix, mcs, s = image_streams(name)[0]
        for _ in range(70):
            m = bytearray(s)
            m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
            streams.append((npix, mcs, bytes(m)))
        streams += [(max(1, npix - 7), mcs, s), (npix + 5, mcs, s), (npix, 2 + (mcs - 1) % 7, s)]    # other sizes, another code size
    early, invalid = C.corrupt_streams()
    streams += [early, invalid]
    whole = run_walker(walker, tmp_path, streams)
    errors = 0
    for (npix, _, _), (err, size, _, _) in zip(streams, whole):
        assert err != 0 or size == npix
        assert size <= npix
        errors += err != 0
    assert errors >= len(streams) // 4
    assert whole[-2][0] == 4 and whole[-1][0] == 1                                  # csm_lzw.h: kErrEarly, kErrCode
    assert run_walker(walker, tmp_path, streams, 16, 3) == whole                    # the same answers through a small window and batch
