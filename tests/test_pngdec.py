"""CPU: the contract of the PNG decoder.  The numpy restatement (tests/pngdec_restatement.py) equals zlib on the raw
bytes and imread on the pixels of every file of tests/pngdec_cases.py; pngread.probe accepts and refuses what it should; the set of
files has the deflate properties it is there for; and the symbol walker of the kernels (csrc/csm_inflate.h), built for the host
under the address and undefined-behaviour sanitizers as a program of its own, agrees on valid streams and stays inside its buffers
on truncated and mutated ones."""
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngdec_cases as C  # noqa: E402
import pngdec_restatement as R  # noqa: E402
from cartoonsegmentation_amd import pngread  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMREAD_MAX_ABS_DIFF = 0          # PNG is lossless: the contract is equality


@pytest.fixture(scope="module")
def decoded():
    return {name: R.decode(C.case_file(name)) for name in C.NAMES}


def stream_of(data):
    return b''.join(body for kind, body in R.chunks(data) if kind == b'IDAT')


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_equals_zlib_and_imread(name, decoded):
    data = C.case_file(name)
    raw, px, stats, (W, H, ct) = decoded[name]
    assert raw.tobytes() == zlib.decompress(stream_of(data))
    ref = C.reference(name)
    assert px.shape == ref.shape == (H, W, 3)
    diff = int(np.abs(px.astype(np.int64) - ref.astype(np.int64)).max())
    print("%s: max |restatement - imread| = %d, %d doubling rounds, blocks %s" % (name, diff, stats['rounds'], stats['blocks']))
    assert diff <= IMREAD_MAX_ABS_DIFF


@pytest.mark.parametrize("name", C.NAMES)
def test_probe_accepts_every_case(name, decoded):
    data = C.case_file(name)
    info = pngread.probe(data)
    _, _, stats, (W, H, ct) = decoded[name]
    assert (info['width'], info['height'], info['colour_type'], info['channels']) == (W, H, ct, R.CHANNELS[ct])
    assert pngread.zlib_stream(data, info).tobytes() == stream_of(data)
    assert info['stream_bytes'] == len(stream_of(data)) and info['adler'] == int.from_bytes(stream_of(data)[-4:], 'big')
    assert (info['adler'] == stats['adler']) == (stats['trailing'] == 0)     # the trailer, unless bytes follow it
    assert (stats['trailing'] > 0) == (name == 'trailing')
    pal = [body for kind, body in R.chunks(data) if kind == b'PLTE']
    assert info['palette'].shape == (256, 3) and info['palette'].dtype == np.uint8
    if pal:
        n = len(pal[0]) // 3
        assert info['palette'][:n].tobytes() == pal[0] and not info['palette'][n:].any()
    d = pngread.descriptor(info, 768, 0, 1 << 33)
    assert d.dtype == np.int32 and d.shape == (pngread.DESC_WORDS,) and (int(d[7]) | int(d[8]) << 31) == 1 << 33
    assert not d[9:].any() and d[6] == 0


def test_probe_reads_no_payload():
    """the deflate data replaced by other bytes (CRCs recomputed): the same description, because nothing in it was interpreted"""
    for name in ('cartoon', 'idat_prime', 'palette7'):
        data = C.case_file(name)
        info = pngread.probe(data)
        out = bytearray(data[:8])
        total, seen = info['stream_bytes'], 0
        for kind, body in R.chunks(data):
            if kind == b'IDAT':
                body = bytes(b if (seen + k < 2 or seen + k >= total - 4) else 0xA5 for k, b in enumerate(body))
                seen += len(body)
            out += C.chunk(kind, body)
        other = pngread.probe(bytes(out))
        assert bytes(out) != data
        for key in ('width', 'height', 'colour_type', 'idat', 'stream_bytes', 'adler', 'orientation'):
            assert other[key] == info[key]
        assert np.array_equal(other['palette'], info['palette'])


@pytest.mark.parametrize("name", sorted(C.REFUSED))
def test_probe_refuses_with_the_reason(name):
    build, word = C.REFUSED[name]
    with pytest.raises(pngread.Unsupported) as e:
        pngread.probe(build())
    assert word in str(e.value), str(e.value)


def test_probe_raises_nothing_else_on_prefixes_and_mutations():
    rng = np.random.default_rng(5)
    for name in ('ancillary', 'palette_trns', 'idat_empty'):
        data = C.case_file(name)
        for n in range(len(data)):
            with pytest.raises(pngread.Unsupported):
                pngread.probe(data[:n])
        for _ in range(300):
            m = bytearray(data)
            m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
            try:
                pngread.probe(bytes(m))
            except pngread.Unsupported:
                pass


def test_the_set_has_its_deflate_properties(decoded):
    st = {name: decoded[name][2] for name in C.NAMES}
    kinds = set()
    for s in st.values():
        kinds |= set(s['blocks'])
    assert kinds == {0, 1, 2}
    assert st['stored']['blocks'].count(0) >= 1 and set(st['fixed']['blocks']) == {1}
    b = st['blocks']['blocks']
    assert b.count(2) >= 4 and b.count(1) >= 1, b
    assert st['flushes']['empty_stored'] >= 4
    assert st['huffman_only']['literal_only_dynamic'] >= 1 and len(st['huffman_only']['matches']) == 0
    m = st['rle']['matches']
    assert len(m) > 10 and (m[:, 2] == 1).all()
    m = st['cartoon']['matches']
    assert (m[:, 1] == 258).any() and (m[:, 2] == 1).any()
    assert (st['far']['matches'][:, 2] >= 16384).any()
    assert st['trailing']['trailing'] > 0 and all(s['trailing'] == 0 for name, s in st.items() if name != 'trailing')
    _, raw, tokens = C.hand_assembled()
    m = st['hand']['matches']
    assert st['hand']['blocks'] == [1] and [tuple(int(v) for v in r) for r in m] == tokens
    assert tuple(m[0, 1:]) == (3, 1)
    far = int(np.flatnonzero(m[:, 2] == 32768)[0])
    assert tuple(m[far, 1:]) == (258, 32768) and tuple(m[far + 1, 1:]) == (258, 1)
    assert decoded['hand'][0].tobytes() == raw
    assert st['deep']['rounds'] >= 10
    assert max(s['rounds'] for s in st.values()) >= 10
    print({name: s['rounds'] for name, s in st.items()})


def test_the_set_has_its_png_properties(decoded):
    filters = {name: decoded[name][0].reshape(decoded[name][3][1], -1)[:, 0] for name in C.NAMES}
    for t in range(5):
        assert any(f[0] == t for f in filters.values()) and any((f[1:] == t).any() for f in filters.values())
    for ct in (0, 4, 2, 6):
        assert set(filters['cycle_ct%d' % ct]) == {0, 1, 2, 3, 4}
    sizes = {decoded[name][3][:2] for name in C.NAMES}
    assert {(1, 1), (1, 37), (37, 1), (3, 1030), (200, 300)} <= sizes and {1, 2, 3, 5} <= {w for w, _ in sizes}
    assert {decoded[name][3][2] for name in C.NAMES} == {0, 2, 3, 4, 6}
    for name, entries in (('palette256', 256), ('palette7', 7), ('palette_trns', 16)):
        kinds = dict(R.chunks(C.case_file(name)))
        assert len(kinds[b'PLTE']) == 3 * entries
        raw, _, _, (W, H, _) = decoded[name]
        assert R.unfilter(raw, H, W, 1).max() < entries
    assert b'tRNS' in dict(R.chunks(C.case_file('palette_trns')))
    for name in ('cycle_ct4', 'cycle_ct6', 'natural'):
        raw, _, _, (W, H, ct) = decoded[name]
        alpha = R.unfilter(raw, H, W, R.CHANNELS[ct]).reshape(H, W, -1)[:, :, -1]
        assert len(np.unique(alpha)) > 1
    sizes = lambda name: [len(body) for kind, body in R.chunks(C.case_file(name)) if kind == b'IDAT']  # noqa: E731
    assert set(sizes('idat_1')) == {1} and set(sizes('idat_prime')[:-1]) == {7} and sizes('idat_empty').count(0) >= 3


# ---- the walker of the kernels, on the host -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("walker") / "inflate_host_check"
    # the sanitizer runtimes are linked statically: the program then needs nothing of them at load time, whatever the environment
    # it inherits preloads
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
           "-I", os.path.join(ROOT, "cartoonsegmentation_amd", "csrc"), os.path.join(ROOT, "tools", "inflate_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run_walker(exe, tmp_path, streams, window=0):
    """[(error word, bytes, adler)] of (raw size, zlib stream) pairs, one process for all of them; window: the bytes of the staging
    window the walker reads through (0: the whole stream)"""
    lines = []
    for k, (raw_size, s) in enumerate(streams):
        p = tmp_path / ("s%d.z" % k)
        p.write_bytes(s)
        lines.append("%d %s\n" % (raw_size, p))
    r = subprocess.run([exe] + (["-w", str(window)] if window else []) + ["-"], input="".join(lines), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(streams)
    return [(int(e), int(n), int(a, 16)) for e, n, a in rows]


def test_walker_equals_the_restatement_on_every_case(walker, tmp_path, decoded):
    streams = [(decoded[name][0].size, stream_of(C.case_file(name))) for name in C.NAMES]
    for window in (0, 1024, 16384):                  # 16384 is the kernel's window; 1024 restages often
        for name, got in zip(C.NAMES, run_walker(walker, tmp_path, streams, window)):
            raw = decoded[name][0]
            assert got == (0, raw.size, zlib.adler32(raw.tobytes())), (name, window)


def test_walker_on_truncated_and_mutated_streams(walker, tmp_path, decoded):
    """every prefix of a few streams and a few hundred seeded single-byte mutations: a clean exit with a non-zero error word or the
    right size, and no sanitizer report (run_walker asserts an empty stderr)"""
    rng = np.random.default_rng(11)
    streams = []
    for name in ('fixed', 'flushes', 'stored', 'width5'):
        s, n = stream_of(C.case_file(name)), decoded[name][0].size
        streams += [(n, s[:k]) for k in range(len(s))]
    for name in ('blocks', 'cartoon', 'hand', 'rle', 'huffman_only', 'palette7'):
        s, n = stream_of(C.case_file(name)), decoded[name][0].size
        for _ in range(80):
            m = bytearray(s)
            m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
            streams.append((n, bytes(m)))
        streams += [(max(0, n - 7), s), (n + 5, s)]              # a raw size that is too small, and one that is too large
    whole = run_walker(walker, tmp_path, streams)
    errors = 0
    for (n, s), (err, size, _) in zip(streams, whole):
        assert err != 0 or size == n
        assert size <= n
        errors += err != 0
    assert errors >= len(streams) // 2
    assert run_walker(walker, tmp_path, streams, 1024) == whole        # the same answers through a small staging window
