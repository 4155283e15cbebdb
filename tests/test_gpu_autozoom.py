"""GPU: the coverage counts of the autozoom search (csrc/autozoom.hip) are, candidate by candidate, the counts of the numpy
restatement (tests/autozoom_restatement.py) on the cases of tests/autozoom_cases.py -- through the LDS band path and through the
plane path, at the default and at ragged chunk sizes.  Every comparison is an equality of integers."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import autozoom_cases as K  # noqa: E402
import autozoom_restatement as A  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from cartoonsegmentation_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def band_supported(H, W):
    from cartoonsegmentation_amd import _lib
    return int(_lib.load().csm_autozoom_band_supported(_lib.i32(H), _lib.i32(W)))


def coverage(ops, c, path, chunk=None, host=True):
    os.environ['CSM_AUTOZOOM_PATH'] = path
    if chunk:
        os.environ['CSM_AUTOZOOM_CHUNK'] = str(chunk)
    try:
        return ops.autozoom_coverage(dev(c['pts'][None]), c['shifts'], c['W'], c['H'], c['focal'], c['baseline'], host=host)
    finally:
        os.environ.pop('CSM_AUTOZOOM_CHUNK', None); os.environ.pop('CSM_AUTOZOOM_PATH', None)


def same_counts(got, want, name, path):
    """integer equality, candidate by candidate; the message names the case, the path, the first candidate that differs and both counts"""
    assert isinstance(got, list) and all(type(v) is int for v in got), (name, path, got)
    assert len(got) == len(want), "%s, %s: %d counts for %d candidates" % (name, path, len(got), len(want))
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    if bad:
        k = bad[0]
        raise AssertionError("%s, %s: %d of %d candidates differ; candidate %d (shift %s): got %d, restated %d" % (
            name, path, len(bad), len(want), k, K.case(name)['shifts'][k], got[k], want[k]))


@pytest.mark.parametrize("name", K.CASES)
def test_band_path_counts_are_the_restated_counts(ops, name):
    c = K.case(name)
    # the path that answers: 1 -- the band kernels really run; 0 -- band_geom refuses the size and the plane path answers
    assert band_supported(c['H'], c['W']) == c['band'], "%s: csm_autozoom_band_supported(%d, %d)" % (name, c['H'], c['W'])
    for call in (1, 2):                                      # the second call allocates its scratch where the first one left it
        same_counts(coverage(ops, c, 'bands'), list(K.restated(name)), name, "bands, call %d" % call)


@pytest.mark.parametrize("name", K.CASES)
def test_plane_path_counts_are_the_restated_counts(ops, name):
    c = K.case(name)
    for chunk in c['chunks']:
        same_counts(coverage(ops, c, 'planes', chunk), list(K.restated(name)), name, "planes, chunk %s" % (chunk or 'default'))


def test_overflow_raises_the_flag_and_the_fallback_is_exact(ops):
    c, want = K.case('pileup'), list(K.restated('pileup'))
    n = len(c['shifts'])
    assert band_supported(c['H'], c['W']) == 1 and c['overflow']
    out = coverage(ops, c, 'bands', host=False)              # on the device: K counts and the overflow flag
    assert out.shape == (n + 1,) and int(out[n]) == 1, "pileup: overflow flag %d" % int(out[n])
    first = coverage(ops, c, 'bands')                        # on the host: the flag sends the call to the plane path
    same_counts(first, want, 'pileup', 'bands -> planes')
    same_counts(coverage(ops, c, 'bands'), first, 'pileup', 'bands -> planes, repeated')
    same_counts(coverage(ops, c, 'bands'), first, 'pileup', 'bands -> planes, repeated twice')
    for name in ('hand_seam', 'group_1x17'):                 # an ordinary case right after the overflow, in the same process
        o = K.case(name)
        out = coverage(ops, o, 'bands', host=False)
        assert int(out[len(o['shifts'])]) == 0, "%s after pileup: overflow flag" % name
        same_counts(out[:len(o['shifts'])].tolist(), list(K.restated(name)), name, 'bands after an overflow')


def test_search_takes_the_first_candidate_with_the_best_count(ops):
    """process_autozoom: the crop filter's candidates, their counts, and the reference's strict `<` (common.py:128-135): among
    several candidates with the best count the first one wins"""
    s = K.search_case()
    cands, shifts = K.search_candidates(s)
    want = A.coverage_counts(s['pts'], shifts, s['H'], s['W'], K.FOCAL, K.BASELINE)
    first = want.index(max(want))
    assert want.count(max(want)) > 1 and first > 0
    common = dict(s['common'], tenRawPoints=dev(s['pts'][None]))
    oF = s['settings']['objFrom']
    for path in ('bands', 'planes'):
        os.environ['CSM_AUTOZOOM_PATH'] = path
        try:
            to, got_cands, counts = ops.process_autozoom(s['settings'], common, return_counts=True)
        finally:
            os.environ.pop('CSM_AUTOZOOM_PATH', None)
        assert got_cands == cands, path
        bad = [k for k in range(len(want)) if counts[k] != want[k]]
        assert len(counts) == len(want) and not bad, "search, %s: candidate %d %s: got %d, restated %d" % (
            path, bad[0], cands[bad[0]], counts[bad[0]], want[bad[0]])
        assert to == {'fltCenterU': oF['fltCenterU'] + cands[first][0], 'fltCenterV': oF['fltCenterV'] + cands[first][1],
                      'intCropWidth': int(round(oF['intCropWidth'] / s['settings']['fltZoom'])),
                      'intCropHeight': int(round(oF['intCropHeight'] / s['settings']['fltZoom']))}, (path, to, cands[first])
