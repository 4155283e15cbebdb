"""CPU: the host side of the JPEG decoder (cartoonsegmentation_amd/jpegcode.py) and the numpy restatement of its contract
(tests/jpegdec_restatement.py) against the project's own encoder, against itself at several subsequence sizes, and
against an independent decoder (PIL / libjpeg)."""
import io
import os
import sys

import numpy as np
import pytest

Image = pytest.importorskip("PIL.Image")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegdec_cases as C  # noqa: E402
import jpegdec_restatement as R  # noqa: E402
import mjpeg_restatement as ENC  # noqa: E402
from cartoonsegmentation_amd import jpegcode  # noqa: E402

# Measured over every file below: the restatement's pixels equal PIL's (libjpeg-turbo's default decode: the accurate integer
# inverse DCT, triangle upsampling, 16-bit colour tables) in every byte.  Both sides are deterministic integer code, so no margin.
PIL_MAX_ABS_DIFF = 0
SUBSEQ_SIZES = (4, 16, 128)


def library_subseq_bytes():
    from cartoonsegmentation_amd import _lib
    return int(_lib.load().csm_jpeg_decode_subseq_bytes())


# ---- probe -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_probe_accepts_every_case(case):
    data = C.case_file(case)
    info = jpegcode.probe(data)
    assert (info['height'], info['width']) == (case['H'], case['W'])
    assert len(info['components']) == (1 if case['mode'] == 'grey' else 3)
    y = info['components'][0]
    assert (y['h'], y['v']) == {'grey': (1, 1), '444': (1, 1), '422': (2, 1), '420': (2, 2)}[case['mode']]
    mx = -(-case['W'] // (8 * y['h']))
    assert info['restart_interval'] == {'none': 0, 'mcu1': 1, 'mcu3': 3, 'row': mx}[case['restart']]
    s, e = info['entropy']
    assert data[e:e + 2] == b'\xff\xd9' and data[s - 14 if len(info['components']) == 3 else s - 10:][:2] == b'\xff\xda'
    assert info['orientation'] is None
    for c in info['components']:
        assert c['tq'] in info['qtables'] and (0, c['td']) in info['huffman'] and (1, c['ta']) in info['huffman']


def exif_with_orientation(v):
    ex = Image.Exif()
    ex[0x0112] = v
    return ex.tobytes()


def test_probe_reads_comments_and_exif():
    img = C.frame('cartoon', 24, 40, 2)
    plain = jpegcode.probe(C.pil_jpeg(img, '420'))
    for extra, want in ((dict(comment=b'a comment \xff\xd9 with marker bytes'), None), (dict(exif=exif_with_orientation(6)), 6),
                        (dict(exif=exif_with_orientation(1)), 1)):
        data = C.pil_jpeg(img, '420', **extra)
        info = jpegcode.probe(data)
        assert info['orientation'] == want
        assert info['entropy'][1] - info['entropy'][0] == plain['entropy'][1] - plain['entropy'][0]
        assert info['qtables'] == plain['qtables'] and info['huffman'] == plain['huffman']
    assert b'\xff\xfe' in C.pil_jpeg(img, '420', comment=b'x')


def test_probe_refuses_what_the_decoder_does_not_take():
    img = C.frame('cartoon', 24, 40, 2)
    good = C.pil_jpeg(img, '420')
    reasons = {}
    reasons['progressive'] = C.pil_jpeg(img, '420', progressive=True)
    buf = io.BytesIO()
    Image.fromarray(np.dstack([img, img[:, :, :1]]), 'CMYK').save(buf, 'JPEG')
    reasons['cmyk'] = buf.getvalue()
    reasons['no_eoi'] = good[:-2]
    reasons['cut_segment'] = good[:30]
    reasons['not_jpeg'] = b'\x89PNG\r\n\x1a\n' + good
    odd = bytearray(C.pil_jpeg(img, '444'))
    odd[odd.index(b'\xff\xc0') + 11] = 0x41            # the luminance sampling factors of the frame header: 4x1
    reasons['411'] = bytes(odd)
    got = {}
    for k, data in reasons.items():
        with pytest.raises(jpegcode.Unsupported) as e:
            jpegcode.probe(data)
        got[k] = str(e.value)
        assert got[k]
    assert 'progressive' in got['progressive'] and ('CMYK' in got['cmyk']) and 'EOI' in got['no_eoi'] and 'segment' in got['cut_segment']
    assert 'sampling' in got['411']
    assert len(set(got.values())) == len(got), got


def test_probe_raises_nothing_else_on_prefixes():
    for data in (C.pil_jpeg(C.frame('cartoon', 17, 33, 1), '420', restart='mcu1', exif=exif_with_orientation(3), comment=b'c'),
                 C.pil_jpeg(C.frame('noise', 8, 8, 1), 'grey', optimize=True)):
        accepted = 0
        for n in range(len(data) + 1):
            try:
                jpegcode.probe(data[:n])
                accepted += 1
            except jpegcode.Unsupported:
                pass
        assert accepted >= 1                     # the whole file; a prefix that happens to end in FF D9 would be one more
        jpegcode.probe(data)


def test_huffman_table_of_the_kernels_decodes_every_code():
    info = jpegcode.probe(C.pil_jpeg(C.frame('noise', 40, 48, 3), '444', quality=100))
    for (cls, tid), (bits, vals) in info['huffman'].items():
        lut, maxcode, valoff, v = jpegcode.huffman_table(bits, vals)
        code, k = 0, 0
        for ln in range(1, 17):
            for _ in range(bits[ln - 1]):
                if ln <= 8:
                    e = int(lut[code << (8 - ln)])
                    assert (e >> 8, e & 255) == (ln, vals[k])
                else:
                    assert int(lut[code >> (ln - 8)]) == 0 and code <= maxcode[ln] and v[valoff[ln] + code] == vals[k]
                    assert all((code >> (ln - s)) > maxcode[s] for s in range(9, ln))
                code += 1
                k += 1
            code <<= 1
    assert len(jpegcode.file_tables(info)) == jpegcode.FILE_TABLE_BYTES


# ---- restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in C.CASES if c['enc'] == 'own'], ids=C.case_id)
def test_coefficients_equal_the_encoder_s(case):
    img = C.frame(case['content'], case['H'], case['W'], case['seed'])
    q, _ = ENC.quantised_blocks(img, case['quality'], case['mode'])
    want = np.zeros((q.shape[0] * q.shape[1], 64), np.int64)
    want[:, R.ZIGZAG] = q.reshape(-1, 64)
    _, coef, _ = C.reference(C.case_file(case))
    assert np.array_equal(coef, want)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_subsequence_model_equals_the_serial_decode(case):
    data = C.case_file(case)
    info, coef, _ = C.reference(data)
    for S in SUBSEQ_SIZES:
        for group in (None, 4):                  # one workgroup; workgroups of four lanes, so that the passes between them matter
            got = R.decode_coefficients_subseq(data, S, info, group=group)
            assert np.array_equal(got, coef), (S, group)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_pixels_against_pil(case):
    data = C.case_file(case)
    _, _, px = C.reference(data)
    ref = C.pil_decode(data)
    assert px.shape == ref.shape == (case['H'], case['W'], 3)
    diff = int(np.abs(px.astype(np.int64) - ref.astype(np.int64)).max())
    print("%s: max |restatement - PIL| = %d" % (C.case_id(case), diff))
    assert diff <= PIL_MAX_ABS_DIFF


@pytest.mark.parametrize("kind", C.SPECIAL_KINDS)
def test_files_with_a_property_at_the_library_s_subsequence_size(kind):
    S = library_subseq_bytes()
    data = C.special_file(kind, S)
    assert C.has_property(kind, data, S)
    info, coef, px = C.reference(data)
    assert np.array_equal(R.decode_coefficients_subseq(data, S, info, group=4), coef)
    assert int(np.abs(px.astype(np.int64) - C.pil_decode(data).astype(np.int64)).max()) <= PIL_MAX_ABS_DIFF


def test_content_cases_have_their_corners():
    """the flat file holds dozens of blocks per subsequence; the noise file at quality 100 has 16-bit codes, blocks without EOB and
    blocks longer than a subsequence; the one at quality 30 has ZRL codes"""
    S = library_subseq_bytes()
    flat = next(c for c in C.CASES if c['content'] == 'flat' and c['mode'] == '420')
    info, coef, _ = C.reference(C.case_file(flat))
    assert coef.shape[0] * S / (info['entropy'][1] - info['entropy'][0]) >= 24
    noise = next(c for c in C.CASES if c['content'] == 'noise' and c['mode'] == '444')
    info, coef, _ = C.reference(C.case_file(noise))
    assert any(b[15] for (cls, _), (b, _) in info['huffman'].items() if cls == 1)          # codes of 16 bits
    zz = coef[:, R.ZIGZAG]
    assert (zz[:, 63] != 0).any()                                                          # no EOB
    assert (info['entropy'][1] - info['entropy'][0]) / coef.shape[0] > S                   # a block is longer than a subsequence
    zrl = next(c for c in C.CASES if c['content'] == 'noise' and c['quality'] == 30)
    zz = C.reference(C.case_file(zrl))[1][:, R.ZIGZAG]
    pos = np.arange(1, 64)[None, :]
    nz = zz[:, 1:] != 0
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)
    prev = np.concatenate([np.zeros((zz.shape[0], 1), np.int64), last[:, :-1]], axis=1)
    assert ((pos - prev - 1)[nz] >= 16).any()                                              # a run of 16 zeros: ZRL
