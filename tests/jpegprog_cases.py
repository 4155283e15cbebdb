"""The files of tests/test_jpegprog.py (CPU) and tests/test_gpu_jpegprog.py (GPU): progressive JPEG files made at test time by PIL's
encoder and, for the scan scripts PIL does not write, by tests/jpegprog_writer.py from the coefficients of a PIL file.  Nothing here
reads a fixture."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegprog_restatement as P  # noqa: E402
import jpegprog_writer as WR  # noqa: E402
from jpegdec_cases import frame, pil_decode, pil_jpeg  # noqa: E402,F401

from cartoonsegmentation_amd import jpegcode  # noqa: E402

SIZES = [(1, 1), (8, 8), (17, 33), (33, 17), (24, 40)]                  # (H, W)
MODES = ['grey', '444', '422', '420']
RESTARTS = [dict(), dict(restart_marker_blocks=1), dict(restart_marker_blocks=2), dict(restart_marker_rows=1)]
RESTART_NAMES = ['none', 'mcu1', 'mcu2', 'row']
CONTENTS = [('flat', 1), ('cartoon', 30), ('noise', 100)]                # (content, quality)
WRITER_SIZE = (40, 56)


def _cases():
    out = []
    for si, (H, W) in enumerate(SIZES):
        for mi, mode in enumerate(MODES):
            # every (size, mode) pair; the restart setting and the content rotate with different periods
            ri, ci = (si + mi) % 4, (si + 2 * mi) % 3
            out.append(dict(H=H, W=W, mode=mode, restart=ri, content=CONTENTS[ci][0], quality=CONTENTS[ci][1]))
    # every restart setting with every content, at the size that is no multiple of an MCU in either direction
    for mode in ('420', 'grey'):
        for ri in range(4):
            for content, quality in CONTENTS:
                c = dict(H=17, W=33, mode=mode, restart=ri, content=content, quality=quality)
                if c not in out:
                    out.append(c)
    return out


CASES = _cases()
WRITER_CASES = [(name, content) for name in WR.SCRIPTS for content in ('cartoon', 'noise')]


def case_id(c):
    return "%s-%dx%d-%s-%s-q%d" % (c['content'], c['W'], c['H'], c['mode'], RESTART_NAMES[c['restart']], c['quality'])


def progressive_jpeg(img, mode, quality, **extra):
    return pil_jpeg(img, mode, quality, 'none', progressive=True, **extra)


@functools.lru_cache(maxsize=None)
def _file(key):
    c = dict(key)
    return progressive_jpeg(frame(c['content'], c['H'], c['W'], 5), c['mode'], c['quality'], **RESTARTS[c['restart']])


def case_file(c):
    return _file(tuple(sorted(c.items())))


@functools.lru_cache(maxsize=None)
def writer_file(name, content):
    """a file of the writer under SCRIPTS[name], from the coefficients of a PIL file of `content`; also that PIL file"""
    mode = 'grey' if name.startswith('grey') else '420'
    H, W = WRITER_SIZE
    src = progressive_jpeg(frame(content, H, W, 2), mode, 100 if content == 'noise' else 90)
    info = jpegcode.probe(src, progressive=True)
    return WR.write(info, P.decode_coefficients(src, info), WR.SCRIPTS[name]), src


def all_small_files():
    """[(id, bytes)] of every case and every writer file"""
    return [(case_id(c), case_file(c)) for c in CASES] + [("writer-%s-%s" % nc, writer_file(*nc)[0]) for nc in WRITER_CASES]


# ---- the reference of a file, computed once and shared -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(data):
    info = jpegcode.probe(data, progressive=True)
    snaps = []
    coef = P.decode_coefficients(data, info, snapshots=snaps)
    px = P.R.pixels(info, coef)
    for a in snaps + [coef, px]:
        a.setflags(write=False)
    return info, tuple(snaps), px


def reference(data):
    """(probe's description, the coefficients after every scan, uint8 BGR pixels) of the restatement's serial decode; read-only"""
    return _reference(bytes(data))


PIL_SCRIPT_LEVELS = [[0, 1, 2, 3, 4], [5, 6, 7, 8], [9]]
