"""CPU: the contract of the lossy WebP decoder.  The Python restatement (tests/webplossy_restatement.py) equals PIL
(libwebp) on the pixels of every file of tests/webplossy_cases.py; the set of files has the VP8 and ALPH features it is there for;
webpread.probe(lossy=True) accepts and refuses what it should and is unchanged without the keyword; and the parsers of the kernels
(csrc/csm_vp8dec.h), built for the host under the address and undefined-behaviour sanitizers as a program of its own, agree with the
restatement on valid files and stay inside their buffers on truncated and mutated ones."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_restatement as E  # noqa: E402
import webpdec_cases as LC  # noqa: E402
import webplossy_cases as C  # noqa: E402
import webplossy_restatement as R  # noqa: E402
from cartoonsegmentation_amd import webpread  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def decoded():
    return {name: R.decode(C.case_file(name)) for name in C.NAMES}


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_equals_pil(name, decoded):
    bgra, _ = decoded[name]
    assert np.array_equal(bgra, C.reference_bgra(name))
    assert np.array_equal(bgra[..., :3], C.reference(name))


def test_our_writers_file_has_8_partitions_and_pil_shows_decoded_rgb():
    H, W, quality, seed = C.OWN['own_272x544']
    frame = np.ascontiguousarray(LC.cartoon(H, W, seed)[..., ::-1])
    res = E.encode_frame(frame, quality)
    assert len(res['parts']) == 8 and E.still_file(res['vp8']) == C.case_file('own_272x544')
    assert np.array_equal(E.decoded_rgb(res, H, W)[..., ::-1], C.reference('own_272x544'))


def test_pillow_emits_the_alph_chunks_the_set_counts_on(decoded):
    """filter 0 and 1, compression 1, with and without pre-processing"""
    a100, a50 = decoded['rgba_aq100'][1]['alph'], decoded['rgba_aq50'][1]['alph']
    assert a100[0] == 1 and a50[0] == 1 and {a100[1], a50[1]} == {0, 1} and {a100[2], a50[2]} == {0, 1}


# ---- what the set covers --------------------------------------------------------------------------------------------------------
def test_the_set_has_its_vp8_features(decoded):
    rep = {name: decoded[name][1] for name in C.NAMES}

    def union(key):
        return set().union(*(r[key] for r in rep.values()))
    assert union('ymodes') == {R.DC_PRED, R.TM_PRED, R.V_PRED, R.H_PRED}
    assert union('bmodes') == set(range(10))
    assert union('uvmodes') == {R.DC_PRED, R.TM_PRED, R.V_PRED, R.H_PRED}
    assert any(r['skipped'] for r in rep.values())
    assert any(len(r['segment_qi']) >= 2 for r in rep.values())
    assert any(r['prob_updates'] for r in rep.values()) and any(not r['prob_updates'] for r in rep.values())
    assert union('cats') == {1, 2, 3, 4, 5, 6}
    assert {r['filter'] for r in rep.values()} == {'none', 'simple', 'normal'}
    assert set().union(*(r['hev'] for r in rep.values() if r['filter'] == 'normal')) == {0, 1, 2}
    assert any(r['has_b'] and len(r['ymodes']) for r in rep.values())          # both kinds of macroblock in one file
    # the transcoder's choices
    for name, parts in (('t_parts2', 2), ('t_parts4', 4), ('t_parts8', 8)):
        assert rep[name]['partitions'] == parts
    assert {rep[n]['partitions'] for n in C.NAMES if not n.startswith('t_')} >= {1, 2, 8}
    r = rep['t_seg_absolute']
    assert r['segmentation'] == (1, 1, 1, 1) and r['segments'] == {0, 1, 2, 3} and r['segment_qi'] == {10, 40, 70, 100}
    assert len(r['filter_levels']) >= 3
    r = rep['t_seg_map_only']
    assert r['segmentation'] == (1, 1, 0, 1) and r['segments'] == {0, 1, 2, 3} and r['segment_qi'] == {0}      # libwebp's reading
    r = rep['t_seg_delta']
    assert r['segmentation'] == (1, 1, 1, 0) and r['segments'] == {0, 1, 2, 3} and r['segment_qi'] == {r['qi'] + d for d in (-20, 0, 15, 40)}
    assert len(r['filter_levels']) == 4
    r = rep['t_lf_delta']
    assert r['lf_delta'] == (1, -7, 12) and r['has_b'] and r['ymodes']
    assert any(level + 12 in r['filter_levels'] for level in r['filter_levels'])      # whole-block and sub-block macroblocks of one segment
    assert rep['t_sharp3']['sharpness'] == 3 and rep['t_sharp7']['sharpness'] == 7
    assert rep['t_sharp3']['filter'] == rep['t_sharp7']['filter'] == 'normal'
    assert rep['t_simple_bpred']['filter'] == 'simple' and rep['t_simple_bpred']['has_b']
    assert rep['t_level0']['filter'] == 'none' and rep['t_level63']['filter_levels'] == {63}
    assert rep['t_noskip']['use_skip'] == 0 and rep['own_flat_48x64']['use_skip'] == 1 and rep['own_flat_48x64']['skipped'] >= 4
    assert rep['t_colour_bits']['colour_bits'] == (1, 1)
    r = rep['t_qdeltas']
    assert all(r['qdelta']) and {v > 0 for v in r['qdelta']} == {True, False}
    assert min(r['segment_qi']) + min(r['qdelta']) < 0 and max(r['segment_qi']) + max(r['qdelta']) > 127
    # every ALPH compression x filter, and the chunks around a muxed file
    assert {rep[n]['alph'][:2] for n in C.ALPH_CASES} == {(c, f) for c in (0, 1) for f in range(4)}
    assert rep['vp8x_meta']['alph'] is not None
    # sizes: a diagonal longer than one step of the reconstruction kernel, and nothing else above 320
    sizes = {n: decoded[n][0].shape[:2] for n in C.NAMES}
    assert {sizes['size_%dx%d' % s] for s in C.SIZES} == set(C.SIZES)
    H, W = sizes['long_diagonal']
    assert min((H + 15) // 16, ((W + 15) // 16 + 1) // 2) > C.RECON_MBS_PER_STEP and rep['long_diagonal']['has_b']
    assert all(max(s) <= 320 for n, s in sizes.items() if n not in ('long_diagonal', 'own_272x544'))


# ---- the container parser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_probe_accepts_every_case(name, decoded):
    data = C.case_file(name)
    info = webpread.probe(data, lossy=True)
    bgra, _ = decoded[name]
    assert info['kind'] == 'lossy' and (info['height'], info['width']) == bgra.shape[:2]
    vp8, alph = R.container(data)
    assert data[info['payload'][0]:info['payload'][1]] == vp8 and info['alpha'] == (alph is not None)
    assert (info['alph'] is None) if alph is None else data[info['alph'][0]:info['alph'][1]] == alph
    with pytest.raises(webpread.Unsupported, match="lossy"):
        webpread.probe(data)


@pytest.mark.parametrize("name", sorted(C.REFUSED))
def test_probe_refuses_with_the_reason(name):
    build, word = C.REFUSED[name]
    with pytest.raises(webpread.Unsupported) as e:
        webpread.probe(build(), lossy=True)
    assert word in str(e.value), str(e.value)
    with pytest.raises(webpread.Unsupported):
        webpread.probe(build())


def test_probe_is_unchanged_on_the_lossless_set():
    for name in LC.NAMES:
        data = LC.case_file(name)
        plain, both = webpread.probe(data), webpread.probe(data, lossy=True)
        assert 'kind' not in plain and both.pop('kind') == 'lossless' and both == plain
    for name, (build, word) in LC.REFUSED.items():
        with pytest.raises(webpread.Unsupported) as e:
            webpread.probe(build())
        assert word in str(e.value)


def test_probe_raises_nothing_else_on_prefixes_and_mutations():
    rng = np.random.default_rng(5)
    for data in (C.case_file('vp8x_meta'), C.case_file('size_17x33'), C.REFUSED['exif6'][0]()):
        for n in range(len(data)):
            with pytest.raises(webpread.Unsupported):
                webpread.probe(data[:n], lossy=True)                 # the RIFF length covers the whole file: no prefix holds it
        for _ in range(400):
            m = bytearray(data)
            m[int(rng.integers(0, min(len(m), 160)))] = int(rng.integers(0, 256))
            try:
                webpread.probe(bytes(m), lossy=True)
            except webpread.Unsupported:
                pass


def test_animation_frames_reads_what_write_webp_writes():
    frames = [np.ascontiguousarray(LC.cartoon(20, 24, 50 + k)[..., ::-1]) for k in range(3)]
    streams = [E.encode_frame(f, 70)['vp8'] for f in frames]
    data = E.animation_file(streams, 24, 20, fps=20, order=[0, 1, 2, 1])
    W, H, spans, durations = webpread.animation_frames(data)
    assert (W, H) == (24, 20) and durations == [50] * 4 and [data[s:e] for s, e in spans] == [streams[i] for i in (0, 1, 2, 1)]
    for bad in (C.case_file('size_17x33'), LC.REFUSED['animated'][0](), data[:-3]):
        with pytest.raises(webpread.Unsupported):
            webpread.animation_frames(bad)


# ---- the parsers of the kernels, on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("checker") / "vp8_host_check"
    # the sanitizer runtimes are linked statically: the program then needs nothing of them at load time, whatever the environment
    # it inherits preloads
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
           "-I", os.path.join(ROOT, "cartoonsegmentation_amd", "csrc"), os.path.join(ROOT, "tools", "vp8_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run_checker(exe, tmp_path, items, pixels=True):
    """items: ('V' | 'A', W, H, chunk bytes).  Returns per item the numbers the program printed and, when its error word is 0 and
    `pixels`, what it wrote: for 'V' (records [mbh,mbw,24], coefficients [mbh,mbw,25,16], B G R [H,W,3]), for 'A' the plane [H,W]"""
    lines = []
    for k, (kind, W, H, s) in enumerate(items):
        p = tmp_path / ("s%d.in" % k)
        p.write_bytes(s)
        lines.append("%s %d %d %s %s\n" % (kind, W, H, p, (tmp_path / ("s%d.out" % k)) if pixels else "-"))
    r = subprocess.run([exe, "-"], input="".join(lines), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(rows) == len(items)
    out = []
    for k, ((kind, W, H, _), row) in enumerate(zip(items, rows)):
        got = None
        if pixels and row[0] == 0:
            raw = (tmp_path / ("s%d.out" % k)).read_bytes()
            if kind == 'A':
                got = np.frombuffer(raw, np.uint8).reshape(H, W)
            else:
                mbw, mbh = (int(v) for v in np.frombuffer(raw, np.int32, 2))
                n = mbw * mbh
                got = (np.frombuffer(raw, np.uint8, n * 24, 8).reshape(mbh, mbw, 24),
                       np.frombuffer(raw, np.int16, n * 400, 8 + n * 24).reshape(mbh, mbw, 25, 16),
                       np.frombuffer(raw, np.uint8, H * W * 3, 8 + n * 824).reshape(H, W, 3))
        out.append((row, got))
    return out


HOST_CASES = [n for n in C.NAMES if n not in ('long_diagonal', 'own_272x544')]


def test_checker_equals_the_restatement_on_valid_files(checker, tmp_path):
    items, frames = [], []
    for name in HOST_CASES:
        data = C.case_file(name)
        vp8, alph = R.container(data)
        H, W = C.reference(name).shape[:2]
        _, _, f, coefs = R.decode_vp8(vp8)
        items.append(('V', W, H, vp8))
        frames.append((name, f, coefs))
        if alph is not None:
            items.append(('A', W, H, alph))
            frames.append((name, None, None))
    for (name, f, coefs), (kind, W, H, _), (row, got) in zip(frames, items, run_checker(checker, tmp_path, items)):
        assert row[0] == 0, (name, row)
        if kind == 'A':
            assert np.array_equal(got, C.reference_bgra(name)[..., 3]), name
            continue
        recs, cf, bgr = got
        hdr = f['header']
        assert row[1] == f['nparts'] and row[3] == hdr['prob_updates'], name
        assert row[2] == (0 if hdr['level'] == 0 else 1 if hdr['simple'] else 2), name
        assert row[4:5 + f['nparts']] == f['used'], (name, row, f['used'])              # bytes consumed, per partition
        for mby in range(f['mbh']):
            for mbx in range(f['mbw']):
                m, rec = f['mbs'][mby][mbx], recs[mby, mbx]
                assert rec[0] == m['segment'] and bool(rec[1] & 1) == bool(m['skip']) and bool(rec[1] & 4) == bool(m['is_b']), name
                assert rec[3] == m['uvmode'] and list(rec[4:20]) == list(m['bmodes']), name
                assert m['is_b'] or rec[2] == m['ymode'], name
        assert np.array_equal(cf, coefs), name
        assert np.array_equal(bgr, C.reference(name)), name


def test_checker_on_truncated_and_mutated_streams(checker, tmp_path):
    """every truncation length of two small files and some hundreds of seeded byte mutations: the program terminates without a
    sanitizer report (run_checker asserts that) and returns either an error or a result.  No share of the mutations has to fail: a
    boolean-coded stream has no redundancy to detect them, and the coder's closing bytes may go unread."""
    rng = np.random.default_rng(11)
    truncated, mutated = [], []
    for name in ('size_17x33', 'alph_c1_f3'):
        data = C.case_file(name)
        vp8, alph = R.container(data)
        H, W = C.reference(name).shape[:2]
        truncated += [('V', W, H, vp8[:k]) for k in range(len(vp8))]
        if alph is not None:
            truncated += [('A', W, H, alph[:k]) for k in range(len(alph))]
    for name in ('cartoon_m4_q75', 'photo_m6_q20', 't_parts8', 't_seg_absolute', 'own_37x53', 'rgba_aq50', 'alph_c1_f1', 'alph_c0_f2'):
        data = C.case_file(name)
        vp8, alph = R.container(data)
        H, W = C.reference(name).shape[:2]
        for _ in range(40):
            m = bytearray(vp8)
            for at in (int(rng.integers(10, 40)), int(rng.integers(10, len(m))), int(rng.integers(10, len(m)))):
                m[at] ^= int(rng.integers(1, 256))
            mutated.append(('V', W, H, bytes(m)))
        mutated += [('V', W + 1, H, vp8), ('V', W, H + 16, vp8)]                        # a descriptor that contradicts the header
        if alph is not None:
            for _ in range(40):
                m = bytearray(alph)
                for at in (int(rng.integers(1, min(len(m), 30))), int(rng.integers(1, len(m)))):
                    m[at] ^= int(rng.integers(1, 256))
                mutated.append(('A', W, H, bytes(m)))
    got = run_checker(checker, tmp_path, truncated, pixels=False)
    for (kind, W, H, s), (row, _) in zip(truncated, got):
        if kind == 'V' and len(s) < 10 + (int.from_bytes(s[:3].ljust(3, b'\0'), 'little') >> 5):
            assert row[0] != 0                                      # the first partition is cut: its size says so in plain bytes
    got = run_checker(checker, tmp_path, mutated)
    valid = sum(row[0] == 0 for row, _ in got)
    print("%d of %d mutated streams still decode" % (valid, len(mutated)))
    for (kind, W, H, s), (row, out) in zip(mutated, got):
        assert (out is not None) == (row[0] == 0)
