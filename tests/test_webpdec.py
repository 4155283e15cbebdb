"""CPU: the contract of the lossless WebP decoder.  The Python restatement (tests/webpdec_restatement.py) equals PIL
(libwebp) on the pixels of every file of tests/webpdec_cases.py and of the lossless writer's own restatement; webpread.probe accepts
and refuses what it should; the set of files has the VP8L features it is there for; and the symbol walker of the kernels
(csrc/csm_vp8l.h), built for the host under the address and undefined-behaviour sanitizers as a program of its own, agrees on valid
streams and stays inside its buffers on truncated and mutated ones."""
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webpdec_cases as C  # noqa: E402
import webpdec_restatement as R  # noqa: E402
import webpll_restatement as WL  # noqa: E402
from cartoonsegmentation_amd import webpread  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SKIPPED_MUTATIONS = 0.5      # the share of mutated streams that may still decode without an error


@pytest.fixture(scope="module")
def decoded():
    return {name: R.decode(C.case_file(name)) for name in C.NAMES}


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_equals_pil(name, decoded):
    argb, feat = decoded[name]
    want = C.reference_bgra(name)
    assert R.bgra(argb, feat['alpha']).shape == want.shape
    assert np.array_equal(R.bgra(argb, feat['alpha']), want)
    assert np.array_equal(R.bgr(argb), C.reference(name))
    data = C.case_file(name)
    slack = 8 * len(R.vp8l_chunk(data)) - feat['bits']
    print("%s: %d bytes, %d bits behind the last symbol, %s" % (name, len(data), slack, feat))
    assert 0 <= slack <= 7 + 8                          # the stream is consumed to its end (a chunk may carry one byte of padding)


def test_restatement_equals_pil_on_our_writers_files():
    from PIL import Image
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (1, 1)).astype(np.uint8), rng.integers(0, 256, (37, 53)).astype(np.uint8), C.cartoon(20, 33, 50), C.cartoon(18, 40, 51, 4)]
    for img in images:
        shape = img.shape
        data = WL.encode(img)
        argb, feat = R.decode(data)
        with Image.open(io.BytesIO(data)) as im:
            want = np.asarray(im.convert('RGBA'))[..., [2, 1, 0, 3]]
        assert np.array_equal(R.bgra(argb, feat['alpha']), want)
        assert feat['transforms'] == [2, 0] and feat['alpha'] == (len(shape) == 3 and shape[2] == 4)
        info = webpread.probe(data)
        assert (info['width'], info['height'], info['alpha']) == (shape[1], shape[0], feat['alpha'])
    mask = rng.integers(0, 2, (9, 21)).astype(bool)
    argb, feat = R.decode(WL.encode(mask))
    assert np.array_equal(R.bgr(argb)[..., 0], mask.astype(np.uint8) * 255)


# ---- the container parser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_probe_accepts_every_case(name, decoded):
    data = C.case_file(name)
    info = webpread.probe(data)
    argb, feat = decoded[name]
    assert (info['width'], info['height'], info['alpha']) == (argb.shape[1], argb.shape[0], feat['alpha'])
    assert webpread.payload(data, info).tobytes() == R.vp8l_chunk(data)
    assert info['extended'] == (data[12:16] == b'VP8X')
    d = webpread.descriptor(info, 4096, 1 << 33, 4)
    assert d.dtype == np.int32 and d.shape == (webpread.DESC_WORDS,)
    assert list(d[:6]) == [info['height'], info['width'], int(info['alpha']), 4, 4096, len(R.vp8l_chunk(data))]
    assert (int(d[7]) | int(d[8]) << 31) == 1 << 33 and d[6] == 0 and not d[9:].any()


def test_probe_reads_no_entropy_data():
    for name in ('c37_m4_q75', 'vp8x_meta', 'hand_groups64'):
        data = bytearray(C.case_file(name))
        info = webpread.probe(bytes(data))
        s, e = info['payload']
        data[s + 5:e] = bytes([0xA5]) * (e - s - 5)
        assert webpread.probe(bytes(data)) == info


@pytest.mark.parametrize("name", sorted(C.REFUSED))
def test_probe_refuses_with_the_reason(name):
    build, word = C.REFUSED[name]
    with pytest.raises(webpread.Unsupported) as e:
        webpread.probe(build())
    assert word in str(e.value), str(e.value)


def test_probe_raises_nothing_else_on_prefixes_and_mutations():
    rng = np.random.default_rng(5)
    for data in (C.case_file('vp8x_meta'), C.case_file('c1_m0_q75'), C.REFUSED['exif6'][0](), C.REFUSED['lossy_alpha'][0]()):
        accepted = 0
        for n in range(len(data)):
            try:
                webpread.probe(data[:n])
                accepted += 1
            except webpread.Unsupported:
                pass
        assert accepted == 0                                # the RIFF length covers the whole file: no prefix holds it
        for _ in range(400):
            m = bytearray(data)
            m[int(rng.integers(0, min(len(m), 120)))] = int(rng.integers(0, 256))
            try:
                webpread.probe(bytes(m))
            except webpread.Unsupported:
                pass


# ---- what the set covers --------------------------------------------------------------------------------------------------------
def test_the_set_has_its_vp8l_features(decoded):
    feats = {name: decoded[name][1] for name in C.NAMES}
    pil = {name: f for name, f in feats.items() if not name.startswith('hand_')}
    sequences = {tuple(f['transforms']) for f in feats.values()}
    assert {(), (3,), (2, 0), (0, 1)} <= {tuple(f['transforms']) for f in pil.values()}
    assert {(3, 0), (2, 0, 1)} <= sequences
    assert set().union(*(f['modes'] for f in pil.values())) == set(range(14))
    block_bits = set()
    for f in feats.values():
        block_bits |= set(f['block_bits'].values())
    assert block_bits >= set(range(2, 10)), block_bits
    hit_bits = {f['cache_bits'][-1] for f in feats.values() if f['cache_hits'] and f['cache_bits'][-1]}
    assert hit_bits >= {1, 2, 3, 4, 5, 6, 11}, hit_bits
    assert {f['cache_bits'][-1] for f in pil.values()} >= {0, 6, 8, 9}
    f = feats['hand_cache6']
    assert f['transforms'] == [] and f['cache_hits'] >= 0.9 * f['size'][0] * f['size'][1]
    groups = {f['groups'] for f in feats.values()}
    assert groups >= {1, 2, 3, 4} and max(groups) >= 64 and max(groups) <= C.GROUP_CAP, groups
    assert {f['meta_bits'] for f in feats.values()} >= set(range(2, 8))
    forms = set().union(*(f['forms'] for f in pil.values()))
    assert forms == {'simple1', 'simple2', 'normal', 'normal_max'}
    for kind in ('map', 'beyond', 'overlap'):
        assert any(f['refs'][kind] for f in pil.values()), kind
    palettes = {f['palette']: f['size'][0] for f in feats.values() if f['palette']}
    assert set(palettes) >= {1, 2, 4, 5, 16, 200}
    for n, packing in ((2, 8), (4, 4), (16, 2)):
        assert any(f['palette'] == n and f['size'][0] % packing for f in feats.values()), n
    sizes = {f['size'] for f in feats.values()}
    assert (1, 1) in sizes and any(w == 1 and h > 1 for w, h in sizes) and any(h == 1 and w > 1 for w, h in sizes)
    assert any(h > C.PREDICT_BAND_ROWS and 0 in f['transforms'] for f in feats.values() for w, h in [f['size']])
    assert any(w > C.PREDICT_BAND_ROWS and 0 in f['transforms'] for f in feats.values() for w, h in [f['size']])
    f = feats['hand_small_block']                               # smaller than one block of either transform and of the entropy image
    assert max(f['size']) < 1 << min(f['block_bits'].values()) and f['meta_bits'] == 5
    assert not feats['hand_alpha_residue']['alpha'] and (decoded['hand_alpha_residue'][0] >> 24 != 255).any()
    assert max(w for w, h in sizes) <= 320 and max(h for w, h in sizes) <= 320


# ---- the walker of the kernels, on the host -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("walker") / "vp8l_host_check"
    # the sanitizer runtimes are linked statically: the program then needs nothing of them at load time, whatever the environment
    # it inherits preloads
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
           "-I", os.path.join(ROOT, "cartoonsegmentation_amd", "csrc"), os.path.join(ROOT, "tools", "vp8l_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run_walker(exe, tmp_path, streams, pixels=True):
    """[(error word, groups, bytes used, alpha flag, ARGB array or None)] of (W, H, payload) triples, one process for all of them"""
    lines = []
    for k, (W, H, s) in enumerate(streams):
        p = tmp_path / ("s%d.vp8l" % k)
        p.write_bytes(s)
        lines.append("%d %d %s %s\n" % (W, H, p, (tmp_path / ("s%d.argb" % k)) if pixels else "-"))
    r = subprocess.run([exe, "-"], input="".join(lines), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(rows) == len(streams)
    out = []
    for k, ((W, H, _), row) in enumerate(zip(streams, rows)):
        px = np.fromfile(tmp_path / ("s%d.argb" % k), '<u4').reshape(H, W) if pixels and row[0] == 0 else None
        out.append(tuple(row) + (px,))
    return out


def test_walker_equals_the_restatement_on_every_case(walker, tmp_path, decoded):
    streams = []
    for name in C.NAMES:
        argb = decoded[name][0]
        streams.append((argb.shape[1], argb.shape[0], R.vp8l_chunk(C.case_file(name))))
    for name, (err, groups, used, alpha, px) in zip(C.NAMES, run_walker(walker, tmp_path, streams)):
        argb, feat = decoded[name]
        assert err == 0 and groups == feat['groups'] and alpha == int(feat['alpha']), name
        assert used == (feat['bits'] + 7) // 8, name
        assert np.array_equal(px, argb), name


def test_walker_reports_a_file_over_the_group_cap(walker, tmp_path):
    """a 8 x 8 image holds 4 blocks of 4 x 4: a fifth group is over this file's cap, which is a refusal and not corruption"""
    data = C.write_vp8l(C.argb_of(C.cartoon(8, 8, 60)), meta_bits=2, groups=4, has_alpha=False)
    (err, groups, _, _, px), = run_walker(walker, tmp_path, [(8, 8, R.vp8l_chunk(data))])
    assert err == 0 and groups == 4 and np.array_equal(px, R.decode(data)[0])
    argb = C.argb_of(C.cartoon(8, 8, 60))
    w = C.L.BitWriter()
    w.number(0x2f, 8); w.number(7, 14); w.number(7, 14); w.number(0, 1); w.number(0, 3); w.number(0, 1)
    C._write_image(w, [int(v) for v in argb.reshape(-1)], 8, 8, 0, [0, 1, 2, 4], 2, main=True)
    over = w.tobytes()
    (err, groups, _, _, _), = run_walker(walker, tmp_path, [(8, 8, over)])
    assert err == webpread.ERR_CAP and groups == 5
    with pytest.raises(R.OverCap):
        R.decode_payload(over, group_cap=4)
    assert R.decode_payload(over)[1]['groups'] == 5


def mutations(rng, s, count):
    """mutations of a payload behind its 5-byte header (a changed header is the container parser's business): three bytes change,
    one of them in the first eighth, where the transforms and the code headers stand.  A single changed byte in the pixel data of
    a lossless stream mostly gives another valid stream; this scheme stays below MAX_SKIPPED_MUTATIONS (asserted below)"""
    out = []
    for _ in range(count):
        m = bytearray(s)
        for at in (int(rng.integers(5, max(6, len(m) // 8))), int(rng.integers(5, len(m))), int(rng.integers(5, len(m)))):
            m[at] ^= int(rng.integers(1, 256))
        out.append(bytes(m))
    return out


def test_walker_on_truncated_and_mutated_streams(walker, tmp_path, decoded):
    """every prefix of a few streams and a few hundred seeded single-byte mutations: a clean exit with a non-zero error word, or the
    pixels of a stream that is still valid (the restatement then agrees), and no sanitizer report (run_walker asserts that)"""
    rng = np.random.default_rng(11)
    truncated, mutated = [], []
    for name in ('c37_m0_q20', 'hand_green_predictor_cross', 'i4_m2_q75', 'hand_cache3', 'c1_m0_q75'):
        s, (W, H) = R.vp8l_chunk(C.case_file(name)), decoded[name][1]['size']
        truncated += [(W, H, s[:k]) for k in range(0, len(s) - 1, max(1, len(s) // 150))]
    for name in ('c37_m4_q75', 'c37_m6_q100', 'hand_groups64', 'hand_palette_predictor', 'hand_cache11', 'cut_m4_q75', 'i200_m0_q75', 'vp8x_meta'):
        s, (W, H) = R.vp8l_chunk(C.case_file(name)), decoded[name][1]['size']
        mutated += [(W, H, m) for m in mutations(rng, s, 40)]
        mutated += [(W + 1, H, s), (W, H - 1 if H > 1 else 2, s)]          # a descriptor that contradicts the header
    got = run_walker(walker, tmp_path, truncated, pixels=False)
    assert all(row[0] != 0 and not row[0] & webpread.ERR_CAP for row in got)
    got = run_walker(walker, tmp_path, mutated)
    valid = 0
    for (W, H, s), (err, _, _, _, px) in zip(mutated, got):
        if err == 0:
            valid += 1
            if valid <= 25:                                     # the restatement is slow: it judges the first of them
                assert np.array_equal(px, R.decode_payload(s)[0])
        else:
            assert not err & webpread.ERR_CAP or err == webpread.ERR_CAP
    print("%d of %d mutated streams are still valid" % (valid, len(mutated)))
    assert valid <= MAX_SKIPPED_MUTATIONS * len(mutated)
