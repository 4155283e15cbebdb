"""GPU: the layer-program kernels of csrc/netops.hip that are not matrix-pipe convolutions, one by one -- k_dwconv_lds / k_dwconv,
k_maxpool, k_bilinear_rows / k_bilinear<4> / k_bilinear<1>, k_nearest, k_eltwise4 / k_eltwise in all four modes with every activation,
k_attractor, k_logbinom, k_gavgpool32 / k_gavgpool and the four transposes -- against the plain float64 references of
tests/netops_cases.py and, bit for bit, against the oracle, at the edge shapes listed there.  tests/test_netops_references.py proves the
same cases (which kernel each selects, the edge it sits on, the planted fault its reference rejects) on the CPU.

Every op runs as a one-op program with the workspace and the output NaN-filled beforehand: whatever the kernel reads outside its view is
NaN, whatever it leaves unwritten stays NaN, and the other channels of a buffer whose slice it writes must still be NaN afterwards."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netops_cases as C  # noqa: E402
import test_netops_references as R  # noqa: E402


def hip_run(b):
    """-> (output NCHW, {whole-buffer view: [n, h, w, C]})"""
    from cartoonsegmentation_amd.runtime import CompiledProgram
    b.prog.plan()
    cp = CompiledProgram(b.prog, 'cuda')
    cp.workspace.fill_(float('nan'))
    out = torch.full(b.out_shape, float('nan'), device='cuda')
    cp.run(*[torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in b.ext_in], out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ({b.guard[0]: cp.read_view(b.guard[0]).cpu().numpy()} if b.guard else {})


def _run_family(family, cases=None):
    """every case of a family: inside its bound against float64 (or equal), bit-equal to the oracle, the guard channels still NaN"""
    cases = C.FAMILIES[family]() if cases is None else cases
    got, worst = [], 0.0
    for k in cases:
        g = R.result_of(k, hip_run, np.isnan)
        worst = max(worst, R.check_case(k, g, 'hip'))
        o = R.oracle_result(k)
        same = np.array_equal(g, o, equal_nan=True)
        assert same, "%s (%s): differs from the oracle in %d of %d values, the first at %r: %r / %r" % (
            k['name'], ', '.join(C.variant(k)), int((g != o).sum()), g.size, np.argwhere(g != o)[0], g[g != o][:4], o[g != o][:4])
        got.append(g)
    R.summary('hip', family, cases, got)
    print("hip %s: worst error %.3g of its bound" % (family, worst))


def test_dwconv_random_weights_on_both_kernels():
    """k 3 / 5 / 7 / 9 (LDS form; 9 is the largest that fits) and 11 (fallback) x frames 1x1 .. 17x33 around the 8 x 16 tile, pad k // 2, 0
    and k - 1, c 32 / 64 (a second channel block), c 36 / 4, stride 2 and dilation 2 on the generic kernel, n 1 / 2, plain buffers and
    channel slices, with and without bias, act none / silu / prelu; a NaN sample next to a finite one stays where it is"""
    _run_family('dwconv')


def test_dwconv_one_hot_weights_give_the_shifted_input_exactly():
    """channel ch carries a 1 at tap (ch + off) % k^2, every tap in turn: the output is that tap's zero-padded window of the input, to
    the bit -- the tap -> offset map of both kernels at every frame size"""
    _run_family('dwconv_onehot')


def test_maxpool_equals_torch_on_negative_inputs():
    """(k, stride, pad, ceil) of every pooling the nets use, on 1x1 .. 21x18, strictly negative inputs (a padding of 0 would win)"""
    _run_family('maxpool')


@pytest.mark.parametrize("which", ['rows', 'grid_limits', 'narrow'])
def test_bilinear_on_each_kernel(which):
    """rows: k_bilinear_rows at c / 4 in {1, 3, 5, 7, 9, 25}, up and down, 1x1 sources and targets, one axis unchanged, equal sizes, rows of
    fewer than / exactly 256 / 257 / several hundred (pixel, 4 channels) pairs; grid_limits: 65536 output rows and 65536 samples fall back
    to k_bilinear<4>; narrow: 1 and 2 channels at a base that is not 16-byte aligned run k_bilinear<1>.  align_corners both ways, a fused
    prelu with a slope per channel"""
    want = {'rows': 'k_bilinear_rows', 'grid_limits': 'k_bilinear<4>', 'narrow': 'k_bilinear<1>'}[which]
    cases = [k for k in C.bilinear_cases() if C.variant(k) == (want,)]
    assert len(cases) >= 4
    _run_family('bilinear', cases)


def test_nearest_equals_repeat():
    _run_family('nearest')


def test_eltwise_add_cropped_add_scale_copy_act_on_both_kernels():
    """add and copy / act through k_eltwise4 and (2-channel slices at an odd offset) through k_eltwise; the cropped add with the first
    operand one row, one column and both larger at n = 2; scale with one vector per sample: all equal to the float64 result rounded once"""
    _run_family('eltwise')


def test_activations_at_their_edges():
    """relu, silu, prelu, hsigmoid, sigmoid, softplus on +-0, denormals, 2^-20 .. 16, the knees +-3, the softplus switch at 20, +-87 .. 1e4
    and 4096 N(0, 3) values: relu and prelu exact, the others inside the bound of max(|x|, 1), finite everywhere"""
    _run_family('activations')


def test_attractor_update():
    _run_family('attractor')


def test_logbinom_expectation_with_both_clamps_and_both_temperature_ends():
    _run_family('logbinom')


def test_gavgpool_on_both_kernels():
    """1 .. 1000 pixels (fewer than, exactly and more than the 256 partial sums), c 32 / 64 (k_gavgpool32, also as a slice with ld = 40)
    and 36 / 4 (k_gavgpool), n = 2, once around a mean of 1000"""
    _run_family('gavgpool')


@pytest.mark.parametrize("c", C.LAYOUT_CS)
def test_layout_transposes_are_exact_both_ways(c):
    """NCHW -> NHWC -> NCHW of distinct values at 1 .. 130 pixels, n = 2: into the padded buffer of the lowering (padding written as
    zeros) and into a slice of a wider buffer (its neighbours stay NaN); 8 .. 240 channels take the tiled kernels, 7 and 241 the plain"""
    _run_family('layout', [k for k in C.layout_cases() if k['c'] == c])
