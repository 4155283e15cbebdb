"""Torch-facing operators with the reference's signatures, backed by libcsm355.so.

Each function mirrors the reference operator cited in its docstring (paths relative to
/root/reference): same argument meaning, same returned tensors, Python exceptions on error.
Tensors must live on the MI355X; a CPU tensor raises (the reference hard-codes CUDA as well,
SURVEY F5).
"""
import torch

from . import _lib
from ._lib import check, f32, f64, i32, i64, ptr, stream_ptr


def _dev(t, name):
    if not t.is_cuda:
        raise _lib.CsmError("%s must be a device tensor (got %s); libcsm355 has no CPU path" % (name, t.device))
    if t.dtype != torch.float32:
        raise _lib.CsmError("%s must be float32" % name)
    return t.contiguous()


def pointrender_update_zee(tenInput, intWidth, intHeight, fltFocal, fltBaseline, tenZee=None):
    """kernel_pointrender_updateZee -- anime_3dkenburns/models/utils.py:63-149"""
    tenInput = _dev(tenInput, "tenInput")
    B, _, N = tenInput.shape
    if tenZee is None:
        tenZee = tenInput.new_full([B, 1, intHeight, intWidth], 1000000.0)
    check(_lib.load().csm_pointrender_update_zee(ptr(tenInput), i32(B), i64(N), i32(intHeight), i32(intWidth),
                                                 f64(fltFocal), f64(fltBaseline), ptr(tenZee), stream_ptr()), "update_zee")
    return tenZee


def pointrender_degrid(tenZee):
    """kernel_pointrender_updateDegrid (Jacobi form) -- models/utils.py:152-212"""
    tenZee = _dev(tenZee, "tenZee")
    B, _, H, W = tenZee.shape
    out = torch.empty_like(tenZee)
    check(_lib.load().csm_pointrender_degrid(ptr(tenZee), ptr(out), i32(B), i32(H), i32(W), stream_ptr()), "degrid")
    return out


def pointrender_update_output(tenInput, tenData, tenZee, fltFocal, fltBaseline):
    """kernel_pointrender_updateOutput -- models/utils.py:215-313; returns accum [B,C+1,H,W]"""
    tenInput, tenData, tenZee = _dev(tenInput, "tenInput"), _dev(tenData, "tenData"), _dev(tenZee, "tenZee")
    B, C, N = tenData.shape
    _, _, H, W = tenZee.shape
    acc = tenInput.new_zeros([B, C + 1, H, W])
    check(_lib.load().csm_pointrender_update_output(ptr(tenInput), ptr(tenData), ptr(tenZee), i32(B), i32(C), i64(N),
                                                    i32(H), i32(W), f64(fltFocal), f64(fltBaseline), ptr(acc),
                                                    stream_ptr()), "update_output")
    return acc


_RENDER_SCRATCH = {}


def _render_tile_scratch(dev, H, W, N):
    """scratch of the tiled render_pointcloud, one per (device, stream, frame size), grown with the cloud; header zeroed once"""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)            # one set per stream: another frame size replaces it
    have = _RENDER_SCRATCH.get(key)
    if have is None or have[1] < N or have[2] != (H, W):
        L = _lib.load()
        cap = int(N * 1.25) + 1024
        buf = torch.empty((L.csm_warp_tile_scratch_bytes(i32(H), i32(W), i64(cap)) + 3) // 4, dtype=torch.float32, device=dev)
        buf[:(L.csm_warp_tile_header_bytes(i32(H), i32(W)) + 3) // 4].zero_()
        _RENDER_SCRATCH[key] = have = (buf, cap, (H, W))
    return have[0]


def render_pointcloud(tenInput, tenData, intWidth, intHeight, fltFocal, fltBaseline, path=None):
    """render_pointcloud -- anime_3dkenburns/models/utils.py:56-315
    tenInput [B,3,N], tenData [B,C,N] -> (tenRender [B,C,H,W], tenExisting [B,1,H,W]).
    path 'tiled' (default for one cloud on frames of at most 8192 tiles): destination-tile binning + LDS splat in channel groups
    (csm_render_pointcloud_tiled, deterministic); 'atomics': the global-atomic chain (csm_render_pointcloud; CSM_RENDER_PATH selects)."""
    import os
    tenInput, tenData = _dev(tenInput, "tenInput"), _dev(tenData, "tenData")
    B, C, N = tenData.shape
    if tenInput.shape[0] != B or tenInput.shape[1] != 3 or tenInput.shape[2] != N:
        raise _lib.CsmError("render_pointcloud: tenInput must be [B,3,N] matching tenData [B,C,N]")
    L = _lib.load()
    path = path or os.environ.get('CSM_RENDER_PATH', 'tiled')
    assert path in ('tiled', 'atomics')
    render = tenInput.new_empty([B, C, intHeight, intWidth])
    existing = tenInput.new_empty([B, 1, intHeight, intWidth])
    if path == 'tiled' and B == 1 and L.csm_warp_tile_supported(i32(intHeight), i32(intWidth)):
        tenInput, tenData = tenInput.contiguous(), tenData.contiguous()
        check(L.csm_render_pointcloud_tiled(ptr(tenInput), ptr(tenData), i32(C), i64(N), i32(intWidth), i32(intHeight), f64(fltFocal),
                                            f64(fltBaseline), ptr(_render_tile_scratch(tenInput.device, intHeight, intWidth, N)),
                                            ptr(render), ptr(existing), stream_ptr()), "render_pointcloud_tiled")
        return render, existing
    zee = tenInput.new_empty([2, B, intHeight, intWidth])
    acc = tenInput.new_empty([B, C + 1, intHeight, intWidth])
    check(L.csm_render_pointcloud(ptr(tenInput), ptr(tenData), i32(B), i32(C), i64(N), i32(intWidth),
                                  i32(intHeight), f64(fltFocal), f64(fltBaseline), ptr(zee), ptr(acc),
                                  ptr(render), ptr(existing), stream_ptr()), "render_pointcloud")
    return render, existing


def fill_disocclusion(tenInput, tenDepth):
    """fill_disocclusion -- anime_3dkenburns/common.py:145-248"""
    tenInput, tenDepth = _dev(tenInput, "tenInput"), _dev(tenDepth, "tenDepth")
    B, C, H, W = tenInput.shape
    out = torch.empty_like(tenInput)
    nbytes = _lib.load().csm_fill_disocclusion_scratch_bytes(i32(B), i32(H), i32(W))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=tenInput.device)
    check(_lib.load().csm_fill_disocclusion(ptr(tenInput), ptr(tenDepth), ptr(out), i32(B), i32(C), i32(H), i32(W),
                                            ptr(scratch), stream_ptr()), "fill_disocclusion")
    return out


def spatial_filter(tenInput, strType):
    """spatial_filter -- anime_3dkenburns/models/utils.py:9-40: 'laplacian' (the hot-path mode), 'median-3', 'median-5'"""
    L = _lib.load()
    fns = {'laplacian': L.csm_spatial_filter_laplacian, 'median-3': L.csm_spatial_filter_median3, 'median-5': L.csm_spatial_filter_median5}
    if strType not in fns:
        raise ValueError("spatial_filter(%r): the reference knows 'laplacian', 'median-3' and 'median-5' (any other type leaves its "
                         "tenOutput None)" % (strType,))
    tenInput = _dev(tenInput, "tenInput")
    B, C, H, W = tenInput.shape
    out = torch.empty_like(tenInput)
    fn = fns[strType]
    check(fn(ptr(tenInput), ptr(out), i32(B * C), i32(H), i32(W), stream_ptr()), "spatial_filter")
    return out


def depth_to_points(tenDepth, fltFocal):
    """depth_to_points -- anime_3dkenburns/models/utils.py:43-50"""
    tenDepth = _dev(tenDepth, "tenDepth")
    B, _, H, W = tenDepth.shape
    pts = tenDepth.new_empty([B, 3, H, W])
    check(_lib.load().csm_depth_to_points(ptr(tenDepth), ptr(pts), i32(B), i32(H), i32(W), f64(fltFocal), stream_ptr()),
          "depth_to_points")
    return pts


def disparity_to_points(tenDisparity, fltFocal, fltBaseline, eps=0.00001, dmax=None):
    """kenburns_effect.py:929-933 fused: normalised disparity -> depth, valid, points, unaltered.
    dmax: optional 1-element device tensor holding max(tenDisparity) when the caller already has it"""
    d = _dev(tenDisparity, "tenDisparity")
    H, W = d.shape[-2:]
    depth, valid = torch.empty_like(d), torch.empty_like(d)
    pts, un = d.new_empty([1, 3, H, W]), d.new_empty([1, 3, H, W])
    if dmax is None:
        dmax = d.max().reshape(1)                                              # stays on the device: no host sync
    check(_lib.load().csm_disparity_to_points(ptr(d), ptr(dmax), i32(H), i32(W), f64(fltFocal),
                                              f64(fltBaseline), f32(eps), ptr(depth), ptr(valid), ptr(pts), ptr(un), stream_ptr()),
          "disparity_to_points")
    return depth, valid, pts, un


def shift_vector(objSettings, objCommon):
    """scalar part of process_shift -- anime_3dkenburns/common.py:60-72 (python floats, like the reference)"""
    cd = objCommon['objDepthrange'][0] + (objSettings['fltDepthTo'] - objSettings['fltDepthFrom'])
    fu, fv = objCommon['objDepthrange'][2][0], objCommon['objDepthrange'][2][1]
    tu, tv = fu + objSettings['fltShiftU'], fv + objSettings['fltShiftV']
    w2, h2, f = objCommon['intWidth'] / 2.0, objCommon['intHeight'] / 2.0, objCommon['fltFocal']
    fx, fy = ((fu - w2) * cd) / f, ((fv - h2) * cd) / f
    tx, ty = ((tu - w2) * cd) / f, ((tv - h2) * cd) / f
    return [fx - tx, fy - ty, objSettings['fltDepthTo'] - objSettings['fltDepthFrom']]


def _f32x3(shift):
    # FloatTensor rounding of the python floats (common.py:74): float64 -> float32, round to nearest even == numpy's conversion
    return f32(float(_np.float32(shift[0]))), f32(float(_np.float32(shift[1]))), f32(float(_np.float32(shift[2])))


def shift_points(tenPoints, shift):
    """tensor part of process_shift -- common.py:74-81; shift = 3 python floats"""
    tenPoints = _dev(tenPoints, "tenPoints")
    B, _, N = tenPoints.shape
    sx, sy, sz = _f32x3(shift)
    out = torch.empty_like(tenPoints)
    check(_lib.load().csm_process_shift(ptr(tenPoints), ptr(out), i32(B), i64(N), sx, sy, sz, stream_ptr()), "process_shift")
    return out


def process_shift(objSettings, objCommon):
    """process_shift -- anime_3dkenburns/common.py:59-84 -> (tenPoints, tenShift)"""
    shift = shift_vector(objSettings, objCommon)
    pts = objSettings['tenPoints']
    tenShift = torch.tensor(shift, dtype=torch.float32).view(1, 3, 1).to(pts.device)
    return shift_points(pts, shift), tenShift


def resize_u8_linear(img, h, w):
    """cv2.resize(img, (w, h), interpolation=cv2.INTER_LINEAR) of a uint8 HxWxC (or HxW) device tensor -- the resampler of
    utils/io_utils.py:254-274 scaledown_maxsize"""
    if not img.is_cuda or img.dtype != torch.uint8:
        raise _lib.CsmError("resize_u8_linear: uint8 device tensor expected")
    img = img.contiguous()
    C = 1 if img.dim() == 2 else int(img.shape[2])
    out = torch.empty((h, w) if img.dim() == 2 else (h, w, C), dtype=torch.uint8, device=img.device)
    check(_lib.load().csm_resize_u8_linear(ptr(img), i32(img.shape[0]), i32(img.shape[1]), i32(C), i32(h), i32(w), ptr(out),
                                           stream_ptr()), "resize_u8_linear")
    return out


def resize_f32_linear(img, h, w):
    """cv2.resize(img, (w, h), interpolation=cv2.INTER_LINEAR) of a float32 HxWxC (or HxW) device tensor (float masks through
    utils/io_utils.py:254-292, animeinsseg/__init__.py:47)"""
    if not img.is_cuda or img.dtype != torch.float32:
        raise _lib.CsmError("resize_f32_linear: float32 device tensor expected")
    img = img.contiguous()
    C = 1 if img.dim() == 2 else int(img.shape[2])
    out = torch.empty((h, w) if img.dim() == 2 else (h, w, C), dtype=torch.float32, device=img.device)
    check(_lib.load().csm_resize_f32_linear(ptr(img), i32(img.shape[0]), i32(img.shape[1]), i32(C), i32(h), i32(w), ptr(out),
                                            stream_ptr()), "resize_f32_linear")
    return out


def resize_bilinear(x, h, w, align_corners=False):
    """torch.nn.functional.interpolate(x, size=(h, w), mode='bilinear', align_corners=...) of a float32 NCHW device tensor (aten
    upsample_bilinear2d restated: csm_resize_bilinear_planes)"""
    x = _dev(x, "x")
    N, C, H, W = x.shape
    out = torch.empty((N, C, h, w), dtype=torch.float32, device=x.device)
    check(_lib.load().csm_resize_bilinear_planes(ptr(x), i32(N * C), i32(H), i32(W), i32(h), i32(w), i32(1 if align_corners else 0), ptr(out),
                                                 stream_ptr()), "resize_bilinear_planes")
    return out


def mean_std(x):
    """device tensor {x.mean(), x.std(unbiased=False)} over all elements (the statistics of Inpaint.forward / Refine.forward)"""
    x = _dev(x, "x")
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    scratch = torch.empty(_lib.load().csm_mean_std_scratch_bytes(), dtype=torch.uint8, device=x.device)
    check(_lib.load().csm_mean_std(ptr(x), i64(x.numel()), ptr(out), ptr(scratch), stream_ptr()), "mean_std")
    return out


def normalise(x, ms):
    """(x - mean) / (std + 1e-7) with ms = mean_std(...)"""
    x = _dev(x, "x")
    out = torch.empty_like(x)
    check(_lib.load().csm_normalise_mean_std(ptr(x), i64(x.numel()), ptr(ms), ptr(out), stream_ptr()), "normalise_mean_std")
    return out


def denormalise(x, ms, mode=0):
    """x * (std + 1e-7) + mean; mode 1: .clip(0, 1), mode 2: threshold(0, 0)"""
    x = _dev(x, "x")
    out = torch.empty_like(x)
    check(_lib.load().csm_denormalise_mean_std(ptr(x), i64(x.numel()), ptr(ms), i32(mode), ptr(out), stream_ptr()), "denormalise_mean_std")
    return out


def autozoom_coverage(tenPoints, shifts, intWidth, intHeight, fltFocal, fltBaseline, chunk=None, host=True):
    """coverage counts `(tenExisting > 0.0).float().sum()` of render_pointcloud(process_shift(tenPoints, shift_k)) for every
    candidate shift_k = (sx, sy, sz) -- common.py:110-126 -- in batched launches (csm_autozoom_coverage), no colour rendered,
    ONE host read.  All candidates of one search share sz (common.py:92-93).  Returns the K counts as a Python list (host=True,
    the default: the read that replaces the reference's <= 256 `.item()` syncs), or a device tensor (host=False; on the band path
    it has K + 1 entries, the last one being the overflow flag of csm_autozoom_coverage_bands)."""
    import ctypes
    import os
    tenPoints = _dev(tenPoints, "tenPoints")
    assert tenPoints.shape[0] == 1 and tenPoints.shape[1] == 3
    L, K = _lib.load(), len(shifts)
    counts = torch.zeros(max(K, 1), dtype=torch.int32, device=tenPoints.device)
    if K == 0:
        return [] if host else counts[:0]
    # FloatTensor rounding of the python-float shifts (common.py:74): float64 -> float32, round to nearest even == numpy's astype
    s32 = _np.asarray([[float(s[0]), float(s[1]), float(s[2])] for s in shifts], dtype=_np.float64).astype(_np.float32)
    sz = {float(v) for v in s32[:, 2]}
    assert len(sz) == 1, "the candidates of one autozoom search share the z shift"
    xy = (ctypes.c_float * (2 * K)).from_buffer_copy(_np.ascontiguousarray(s32[:, :2]).tobytes())
    path = os.environ.get('CSM_AUTOZOOM_PATH', 'bands')
    if chunk is None and path == 'bands' and L.csm_autozoom_band_supported(i32(intHeight), i32(intWidth)):
        # band path: z-buffers in LDS, candidates grouped by y shift.  The overflow flag travels with the counts (one transfer).
        N = tenPoints.shape[2]
        out = torch.empty(K + 1, dtype=torch.int32, device=tenPoints.device)
        scratch = torch.empty((L.csm_autozoom_band_scratch_bytes(i32(intHeight), i32(intWidth), i64(N)) + 3) // 4, dtype=torch.float32,
                              device=tenPoints.device)
        zs = f32(sz.pop())
        check(L.csm_autozoom_coverage_bands(ptr(tenPoints), i64(N), i32(intHeight), i32(intWidth), f64(fltFocal), f64(fltBaseline), xy,
                                            zs, i32(K), ptr(scratch), ptr(out), ctypes.c_void_p(out.data_ptr() + 4 * K), stream_ptr()),
              "autozoom_coverage_bands")
        if not host:
            return out                                      # [K + 1]: counts, overflow flag (callers that stay on the device check it)
        vals = out.tolist()
        if vals[K] == 0:
            return vals[:K]
        sz = {zs.value}                                     # a band segment overflowed (pathological cloud): exact plane path below
    chunk = int(chunk or os.environ.get('CSM_AUTOZOOM_CHUNK', L.csm_autozoom_max_chunk()))
    chunk = max(1, min(chunk, L.csm_autozoom_max_chunk(), K))
    scratch = torch.empty(L.csm_autozoom_scratch_floats(i32(intHeight), i32(intWidth), i32(chunk)), dtype=torch.float32,
                          device=tenPoints.device)
    check(L.csm_autozoom_coverage(ptr(tenPoints), i64(tenPoints.shape[2]), i32(intHeight), i32(intWidth), f64(fltFocal),
                                  f64(fltBaseline), xy, f32(sz.pop()), i32(K), i32(chunk), ptr(scratch), ptr(counts), stream_ptr()),
          "autozoom_coverage")
    return counts[:K].tolist() if host else counts[:K]


def process_autozoom(objSettings, objCommon, return_counts=False):
    """process_autozoom -- anime_3dkenburns/common.py:86-142: the 16 x 16 grid of candidate shifts whose crop stays inside the
    image, the one with the largest rendered coverage wins (first strictly-better candidate, like the reference's `<`).
    MI355X: all candidates in batched launches + ONE host read instead of <= 256 x (3 kernels + `.item()`)."""
    import numpy as np
    shift = objSettings['fltShift']
    lin = np.linspace(-shift, shift, 16)
    oF = objSettings['objFrom']
    cw, ch = oF['intCropWidth'] / objSettings['fltZoom'], oF['intCropHeight'] / objSettings['fltZoom']
    d_from = objCommon['objDepthrange'][0]
    d_to = objCommon['objDepthrange'][0] * (cw / oF['intCropWidth'])
    cu, cv = oF['fltCenterU'], oF['fltCenterV']
    W, H = objCommon['intWidth'], objCommon['intHeight']
    cands = []
    for iu in range(16):
        for iv in range(16):
            su, sv = lin[iv].item(), lin[iu].item()        # npyShiftU[intU, intV] = lin[intV]; npyShiftV[intU, intV] = lin[intU]
            if cu + su < cw / 2.0 or cu + su > W - (cw / 2.0) or cv + sv < ch / 2.0 or cv + sv > H - (ch / 2.0):
                continue
            cands.append((su, sv))
    shifts = [shift_vector({'fltShiftU': su, 'fltShiftV': sv, 'fltDepthFrom': d_from, 'fltDepthTo': d_to}, objCommon) for su, sv in cands]
    counts = autozoom_coverage(objCommon['tenRawPoints'], shifts, W, H, objCommon['fltFocal'], objCommon['fltBaseline'])
    best, bu, bv = 0.0, None, None
    for (su, sv), c in zip(cands, counts):
        if best < c:
            best, bu, bv = float(c), su, sv
    out = {'fltCenterU': cu + bu, 'fltCenterV': cv + bv,
           'intCropWidth': int(round(oF['intCropWidth'] / objSettings['fltZoom'])),
           'intCropHeight': int(round(oF['intCropHeight'] / objSettings['fltZoom']))}
    return (out, cands, counts) if return_counts else out


class WarpFrame:
    """Fused per-frame warp of KenBurnsPipeline.process_kenburns (kenburns_effect.py:1027-1040):
    process_shift -> render_pointcloud(cat[rgb,depth]) -> fill_disocclusion -> uint8 HWC.
    Owns the scratch so the frame loop allocates nothing.  path 'tiled' (default): destination-tile binning + LDS splat
    (csm_warp_frame_tiled); 'atomics': the global-atomic chain of csm_warp_frame (CSM_WARP_PATH selects)."""

    def __init__(self, H, W, device, keep_render=False, path=None):
        import os
        self.H, self.W, self.device = H, W, device
        self.path = path or os.environ.get('CSM_WARP_PATH', 'tiled')
        assert self.path in ('tiled', 'atomics')
        if self.path == 'tiled' and not _lib.load().csm_warp_tile_supported(i32(H), i32(W)):
            self.path = 'atomics'                          # more than 8192 tiles (e.g. 3840 x 2160): the global-atomic chain has no limit
        self.frame = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
        self.render = torch.empty((1, 4, H, W), dtype=torch.float32, device=device) if keep_render else None
        self.scratch, self._cap = None, -1
        if self.path == 'atomics':
            n = _lib.load().csm_warp_frame_scratch_floats(i32(H), i32(W))
            self.scratch = torch.empty(n, dtype=torch.float32, device=device)

    def _tile_scratch(self, N):
        if N > self._cap:                                  # the point cloud grows when inpainting appends points
            L = _lib.load()
            cap = int(N * 1.25) + 1024
            nbytes = L.csm_warp_tile_scratch_bytes(i32(self.H), i32(self.W), i64(cap))
            self.scratch = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
            hdr = (L.csm_warp_tile_header_bytes(i32(self.H), i32(self.W)) + 3) // 4
            self.scratch[:hdr].zero_()                     # the bin counters must start at zero; every frame re-arms them
            self._cap = cap
        return self.scratch

    def __call__(self, tenPoints, tenImage, tenDepth, fltFocal, fltBaseline, shift, stream=None):
        N = tenPoints.shape[2]
        sx, sy, sz = _f32x3(shift)
        st = stream_ptr() if stream is None else stream
        if self.path == 'tiled':
            check(_lib.load().csm_warp_frame_tiled(ptr(tenPoints), ptr(tenImage), ptr(tenDepth), i64(N), i32(self.H), i32(self.W),
                                                   f64(fltFocal), f64(fltBaseline), sx, sy, sz, ptr(self._tile_scratch(N)),
                                                   ptr(self.render), ptr(self.frame), st), "warp_frame_tiled")
        else:
            check(_lib.load().csm_warp_frame(ptr(tenPoints), ptr(tenImage), ptr(tenDepth), i64(N), i32(self.H), i32(self.W),
                                             f64(fltFocal), f64(fltBaseline), sx, sy, sz, ptr(self.scratch),
                                             ptr(self.render), ptr(self.frame), st), "warp_frame")
        return self.frame, self.render

    def frames(self, tenPoints, tenImage, tenDepth, fltFocal, fltBaseline, shifts, lanes=3, out=None, stream=None):
        """K frames of one cloud in ONE call (csm_warp_frames_tiled): shifts = K x (sx, sy, sz); returns uint8 [K, H, W, 3].  The frames are
        bit-identical to K __call__s; frame k + 1's binning and frame k - 1's hole fill overlap frame k's render on internal streams."""
        import ctypes
        assert self.path == 'tiled'
        L = _lib.load()
        N = tenPoints.shape[2]
        K = len(shifts)
        flat = []
        for s in shifts:
            flat.extend(float(v.value) for v in _f32x3(s))
        arr = (ctypes.c_float * (3 * max(K, 1)))(*flat)
        st = stream_ptr() if stream is None else stream
        if getattr(self, '_multi_key', None) is None or self._multi_key[0] < N or self._multi_key[1] != lanes:
            cap = int(N * 1.25) + 1024                         # (the point cloud grows when inpainting appends points)
            nbytes = L.csm_warp_frames_scratch_bytes(i32(self.H), i32(self.W), i64(cap), i32(lanes))
            self._multi = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=self.device)     # (headers must start at zero)
            self._multi_key = (cap, lanes)
            self._multi_n = N
        elif self._multi_n != N:
            # the library carves lane i at i * round256(csm_warp_tile_scratch_bytes(H, W, N)) with the CURRENT N: when N changes, the
            # headers of lanes 1.. fall into bytes the previous call used as depth / entry storage, and the tile protocol needs every
            # header zero on entry -> clear the buffer on the stream the call runs on
            if stream is None:
                self._multi.zero_()
            else:
                with torch.cuda.stream(torch.cuda.ExternalStream(int(stream.value or 0), device=self.device)):
                    self._multi.zero_()
            self._multi_n = N
        if out is None:
            out = torch.empty((K, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        check(L.csm_warp_frames_tiled(ptr(tenPoints), ptr(tenImage), ptr(tenDepth), i64(N), i32(self.H), i32(self.W), f64(fltFocal),
                                      f64(fltBaseline), arr, i32(K), i32(lanes), ptr(self._multi), ptr(None), ptr(out), st), "warp_frames_tiled")
        return out

    def frame_into(self, out_hwc, tenPoints, tenImage, tenDepth, fltFocal, fltBaseline, shift, patch_h, patch_w, center_x, center_y,
                   dof=None):
        """One output frame of the video loop in ONE library call (csm_kenburns_frame, kenburns_effect.py:1027-1072): warp
        [-> colourised depth -> depth-of-field blur with dof = (focal_plane, num_samples, lightness_factor)] -> crop + resize into
        `out_hwc`.  Same kernels and bits as __call__ + colorize_gray_r + bokeh_blur + csm_crop_resize_u8; tiled path only."""
        import ctypes
        global _GRAY_R_LUT
        assert self.path == 'tiled'
        L = _lib.load()
        if dof is not None:
            assert self.render is not None, "depth of field needs WarpFrame(keep_render=True)"
            if _GRAY_R_LUT is None:
                lut = ((1.0 - _np.linspace(0.0, 1.0, 256)) * 255).astype(_np.uint8)
                _GRAY_R_LUT = (ctypes.c_uint8 * 256)(*[int(x) for x in lut])
            if getattr(self, '_tail', None) is None:
                self._tail = torch.zeros(L.csm_kenburns_frame_scratch_bytes(i32(self.H), i32(self.W)), dtype=torch.uint8, device=self.device)
        N = tenPoints.shape[2]
        sx, sy, sz = _f32x3(shift)
        fp, ns, lf = (0.0, 32, 1.0) if dof is None else (float(_np.float32(dof[0])), int(dof[1]), float(dof[2]))
        check(L.csm_kenburns_frame(ptr(tenPoints), ptr(tenImage), ptr(tenDepth), i64(N), i32(self.H), i32(self.W), f64(fltFocal),
                                   f64(fltBaseline), sx, sy, sz, ptr(self._tile_scratch(N)), ptr(self.render), ptr(self.frame),
                                   i32(0 if dof is None else 1), f32(fp), i32(ns), f32(lf), _GRAY_R_LUT if dof is not None else None,
                                   ptr(getattr(self, '_tail', None)), i32(patch_h), i32(patch_w), f32(center_x), f32(center_y),
                                   ptr(out_hwc), stream_ptr()), "kenburns_frame")


# ---- bokeh depth-of-field (utils/effects.py:143-181, depth_modules/zoedepth/utils/misc.py:97-135) ---------------------
import math as _math

import numpy as _np

_GRAY_R_LUT = None


def _percentile_linear(sorted_vals, q):
    """np.percentile(..., method='linear') on an ascending device tensor (two element reads)"""
    n = sorted_vals.numel()
    vi = (n - 1) * (q / 100.0)
    lo = int(_math.floor(vi)); hi = min(lo + 1, n - 1)
    a, b = float(sorted_vals[lo].item()), float(sorted_vals[hi].item())
    t = vi - lo
    r = a + (b - a) * t if t < 0.5 else b - (b - a) * (1 - t)          # numpy _lerp
    return float(_np.float32(r))


_TAIL_SCRATCH = {}


def image_tensor(img_hwc_u8):
    """uint8 HxWx3 device image -> float32 [1,3,H,W] in [0,1] (`img.permute(2, 0, 1)[None].float() * (1.0 / 255.0)`), one kernel"""
    img = img_hwc_u8
    if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3):
        raise _lib.CsmError("image_tensor: a uint8 HxWx3 device tensor is required; libcsm355 has no CPU path")
    img = img.contiguous()
    H, W = int(img.shape[0]), int(img.shape[1])
    out = torch.empty((1, 3, H, W), dtype=torch.float32, device=img.device)
    check(_lib.load().csm_u8_hwc_to_f32_chw(ptr(img), i32(H), i32(W), ptr(out), stream_ptr()), "u8_hwc_to_f32_chw")
    return out


def _frame_block(B, n, dev, dtype=torch.float32):
    """[B, stride] block for B frames of n elements each, stride = n rounded up to 4 elements: every frame's view starts 16-byte
    aligned like a tensor of its own (csm_minmax and other float4 readers require it)"""
    stride = (n + 3) & ~3
    return torch.empty((B, stride), dtype=dtype, device=dev), stride


def frame_glue_batch(frames, coarse, masks, fltFocal, fltBaseline, eps=0.00001):
    """The per-frame depth glue of B equally sized frames in one native call (csm_frame_glue_batch): image_tensor, the depth
    adjustment for each frame's instances, raw min/max, normalisation, disparity_to_points and the depth crop's minMaxLoc.
    frames: B uint8 [H,W,3] device tensors; coarse: B float32 [1,1,H,W]; masks: B uint8 [n_k,H,W] tensors or None (no instance).
    Returns per-frame VIEWS of block-allocated [B, ...] outputs, with the shapes the per-frame operators hand out, and the
    [B, 6] float64 stats tensor (still on the device: the caller reads it once)."""
    import ctypes
    L = _lib.load()
    B = len(frames)
    H, W = int(frames[0].shape[0]), int(frames[0].shape[1])
    dev, n = frames[0].device, H * W
    for f, c, m in zip(frames, coarse, masks):
        if not (f.is_cuda and f.dtype == torch.uint8 and tuple(f.shape) == (H, W, 3) and f.is_contiguous()):
            raise _lib.CsmError("frame_glue_batch: equally sized contiguous uint8 HxWx3 device frames are required")
        if not (c.is_cuda and c.dtype == torch.float32 and c.numel() == n and c.is_contiguous()):
            raise _lib.CsmError("frame_glue_batch: every coarse disparity must be a contiguous float32 device map of the frame size")
        if m is not None and not (m.is_cuda and m.dtype == torch.uint8 and tuple(m.shape[1:]) == (H, W) and m.is_contiguous()):
            raise _lib.CsmError("frame_glue_batch: masks must be contiguous uint8 [n,H,W] device tensors")
    img, s3 = _frame_block(B, 3 * n, dev)
    pts, un = torch.empty_like(img), torch.empty_like(img)
    disp, s1 = _frame_block(B, n, dev)
    depth, valid = torch.empty_like(disp), torch.empty_like(disp)
    nmax = torch.empty(B, dtype=torch.float32, device=dev)
    stats = torch.empty((B, 6), dtype=torch.float64, device=dev)
    scratch = torch.empty(L.csm_frame_glue_scratch_bytes(i32(B), i32(H), i32(W)), dtype=torch.uint8, device=dev)
    VP = ctypes.c_void_p * B
    counts = [0 if m is None else int(m.shape[0]) for m in masks]
    check(L.csm_frame_glue_batch(i32(B), i32(H), i32(W), VP(*[f.data_ptr() for f in frames]), VP(*[c.data_ptr() for c in coarse]),
                                 VP(*[m.data_ptr() if k else None for m, k in zip(masks, counts)]), (ctypes.c_int * B)(*counts),
                                 f64(fltFocal), f64(fltBaseline), f32(eps), ptr(img), ptr(disp), ptr(depth), ptr(valid), ptr(pts), ptr(un),
                                 i64(s1), i64(s3), ptr(nmax), ptr(stats), ptr(scratch), stream_ptr()), "frame_glue_batch")
    v1 = lambda t, k: t[k, :n].view(1, 1, H, W)
    v3 = lambda t, k: t[k, :3 * n].view(1, 3, H, W)
    return {'image': [v3(img, k) for k in range(B)], 'disparity': [v1(disp, k) for k in range(B)],
            'depth': [v1(depth, k) for k in range(B)], 'valid': [v1(valid, k) for k in range(B)],
            'points': [v3(pts, k) for k in range(B)], 'unaltered': [v3(un, k) for k in range(B)], 'nmax': nmax, 'stats': stats}


def leres_post_batch(y, H, W):
    """LeReS post-processing of the net outputs y [B,1,h,w] in one native call (csm_leres_post_batch): per sample min/max -> uint8
    quantisation -> resize back to H x W -> zero fix.  Returns B views [1,1,H,W] of one block."""
    L = _lib.load()
    y = _dev(y, "y")
    B, h, w = int(y.shape[0]), int(y.shape[-2]), int(y.shape[-1])
    out, stride = _frame_block(B, H * W, y.device)
    scratch = torch.empty(L.csm_leres_post_scratch_bytes(i32(B), i32(h), i32(w)), dtype=torch.uint8, device=y.device)
    check(L.csm_leres_post_batch(ptr(y), i32(B), i32(h), i32(w), i32(H), i32(W), ptr(out), i64(stride), ptr(scratch), stream_ptr()),
          "leres_post_batch")
    return [out[k, :H * W].view(1, 1, H, W) for k in range(B)]


def ctypes_ptr(t, offset_elems):
    """device pointer `offset_elems` elements into tensor t"""
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def _tail_scratch(dev):
    """scratch of the sync-free frame tail (percentile select state + partial histograms, bokeh stats), one set per (device,
    stream): calls on one stream are ordered, calls on different streams / threads of a device get their own state"""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    if key not in _TAIL_SCRATCH:
        L = _lib.load()
        _TAIL_SCRATCH[key] = (torch.zeros(L.csm_percentile_scratch_bytes(), dtype=torch.uint8, device=dev),          # counting tables start cleared
                              torch.zeros(L.csm_bokeh_depth_scratch_bytes(), dtype=torch.uint8, device=dev),   # completion counter starts at 0
                              torch.empty(2, dtype=torch.float32, device=dev))
    return _TAIL_SCRATCH[key]


def colorize_gray_r(tenValue):
    """colorize(value, cmap='gray_r')[..., 0] -> uint8 tensor (same shape, squeezed); vmin/vmax = 2nd / 85th percentile
    (depth_modules/zoedepth/utils/misc.py:97-135).  No sort and no host sync: the percentiles are selected on the device
    (csm_percentile_pair) and consumed from device memory."""
    global _GRAY_R_LUT
    import ctypes
    v = _dev(tenValue.reshape(-1), "tenValue")
    L = _lib.load()
    if _GRAY_R_LUT is None:
        # matplotlib: lut = 1 - linspace(0,1,256) (float64); bytes=True -> (lut*255).astype(uint8)  [truncation, not 255-k]
        lut = ((1.0 - _np.linspace(0.0, 1.0, 256)) * 255).astype(_np.uint8)
        _GRAY_R_LUT = (ctypes.c_uint8 * 256)(*[int(x) for x in lut])
    sel, _, vmm = _tail_scratch(v.device)
    check(L.csm_percentile_pair(ptr(v), i64(v.numel()), f64(2.0), f64(85.0), ptr(vmm), ptr(sel), stream_ptr()), "percentile_pair")
    out = torch.empty(v.numel(), dtype=torch.uint8, device=v.device)
    check(L.csm_colorize_gray_r_dev(ptr(v), ptr(out), i64(v.numel()), ptr(vmm), _GRAY_R_LUT, stream_ptr()), "colorize")
    return out.reshape(tenValue.squeeze().shape)


def bokeh_blur(img, depth, num_samples=32, lightness_factor=10, depth_factor=2, use_cuda=False, focal_plane=None):
    """bokeh_blur -- utils/effects.py:143-181.  img uint8 HxWx3 and depth uint8/float HxW as device tensors (numpy inputs are
    uploaded); returns a uint8 HxWx3 DEVICE tensor.  `use_cuda` is accepted for signature compatibility (always device)."""
    L = _lib.load()
    dev = img.device if isinstance(img, torch.Tensor) else torch.device('cuda', torch.cuda.current_device())
    img_d = (img if isinstance(img, torch.Tensor) else torch.from_numpy(_np.ascontiguousarray(img))).to(dev).contiguous()
    H, W = int(img_d.shape[0]), int(img_d.shape[1])
    n = H * W
    d8 = (depth if isinstance(depth, torch.Tensor) else torch.from_numpy(_np.ascontiguousarray(depth))).to(dev)
    if d8.dtype not in (torch.uint8, torch.float32):
        d8 = d8.float()                                    # `depth.astype(np.float32)`, utils/effects.py:147
    d8 = d8.contiguous()
    dm = torch.empty((H, W), dtype=torch.float32, device=dev)
    if d8.dtype == torch.uint8 and depth_factor == 1 and focal_plane is not None:
        # the pipeline's call (uint8 colorized depth, configs/3dkenburns.yaml:47): depth.max(), min / max of depth.max() - |depth - focal|
        # (utils/effects.py:146-153) in closed form from the uint8 histogram, on the device
        fp = float(_np.float32(focal_plane))
        check(L.csm_bokeh_depth_auto(ptr(d8), ptr(dm), i64(n), f32(fp), ptr(_tail_scratch(dev)[1]), stream_ptr()), "bokeh_depth")
    else:
        # the reference's general form, incl. its own defaults (float depth, depth_factor = 2, focal_plane = None)
        tmp = torch.empty(n + 4 + 512, dtype=torch.float32, device=dev)
        check(L.csm_bokeh_depth_general(ptr(d8), i32(1 if d8.dtype == torch.uint8 else 0), i64(n), i32(0 if focal_plane is None else 1),
                                        f32(0.0 if focal_plane is None else float(_np.float32(focal_plane))), f32(float(depth_factor)),
                                        ptr(tmp), ctypes_ptr(tmp, n), ctypes_ptr(tmp, n + 4), ptr(dm), stream_ptr()), "bokeh_depth_general")
    hi = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    check(L.csm_bokeh_highlight(ptr(img_d), ptr(hi), i64(n * 3), f32(lightness_factor), stream_ptr()), "bokeh_highlight")
    a, b = torch.empty_like(hi), torch.empty_like(hi)
    PI = _math.pi
    for src, dst, (dx, dy) in ((hi, a, (0, 1)), (a, b, (_math.cos(-PI / 6), _math.sin(-PI / 6)))):
        check(L.csm_bokeh_pass(ptr(src), ptr(dm), ptr(dst), i32(H), i32(W), i32(num_samples), f32(dx), f32(dy), stream_ptr()), "bokeh_pass")
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    # third pass + ((diag + rhom) / 2) ** (1 / lightness) * 255 -> uint8 (utils/effects.py:172,179-180) in one kernel
    check(L.csm_bokeh_pass_finish(ptr(b), ptr(dm), ptr(out), i32(H), i32(W), i32(num_samples), f32(_math.cos(-PI * 5 / 6)),
                                  f32(_math.sin(-PI * 5 / 6)), f32(lightness_factor), stream_ptr()), "bokeh_pass_finish")
    return out


def mask_rle_encode(masks):
    """COCO compressed RLE of bool / uint8 device masks [n,H,W] (or one [H,W]): the 'counts' strings of
    pycocotools.mask.encode (utils/io_utils.py:327-333 mask2rle; any non-zero byte is set) and the pixel counts.  Returns
    (counts: list of str, areas: int64 numpy [n]).  The strings are built on the device (csm_mask_rle_measure / _write); the
    host reads the small info array once, then only the characters."""
    if not (isinstance(masks, torch.Tensor) and masks.is_cuda):
        raise _lib.CsmError("mask_rle_encode: masks must be a device tensor; libcsm355 has no CPU path")
    if masks.dtype not in (torch.bool, torch.uint8) or masks.dim() not in (2, 3):
        raise _lib.CsmError("mask_rle_encode: bool or uint8 masks [n,H,W] or [H,W] expected (got %s %s)" % (masks.dtype, tuple(masks.shape)))
    L = _lib.load()
    m = masks.contiguous()                                  # named: alive until the kernels that read it are enqueued
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    if m.dim() == 2:
        m = m.unsqueeze(0)
    n, H, W = (int(v) for v in m.shape)
    if n == 0:
        return [], _np.zeros(0, _np.int64)
    if H * W > 2 ** 31 - 1:
        raise _lib.CsmError("mask_rle_encode: H*W must stay below 2^31 (got %dx%d)" % (H, W))
    dev = m.device
    info = torch.empty((n, 4), dtype=torch.int64, device=dev)
    scratch = torch.empty(L.csm_mask_rle_scratch_bytes(i32(n), i32(H), i32(W)), dtype=torch.uint8, device=dev)
    st = stream_ptr(dev)
    check(L.csm_mask_rle_measure(ptr(m), i32(n), i32(H), i32(W), ptr(info), ptr(scratch), st), "mask_rle_measure")
    info_h = info.cpu().numpy()                             # the one sync before the strings are sized
    total = int(info_h[-1, 3] + info_h[-1, 1])
    chars = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    check(L.csm_mask_rle_write(ptr(m), i32(n), i32(H), i32(W), ptr(info), ptr(chars), ptr(scratch), st), "mask_rle_write")
    blob = chars[:total].cpu().numpy().tobytes()
    counts = [blob[o:o + b].decode('ascii') for o, b in zip(info_h[:, 3].tolist(), info_h[:, 1].tolist())]
    return counts, info_h[:, 2].copy()


# ---- host scaffolding the codec wrappers below share ------------------------------------------------------------------------
def _byte_files(files, what):
    """(single, datas): one `bytes`-like file, or a list of them"""
    single = isinstance(files, (bytes, bytearray, memoryview))
    datas = [files] if single else list(files)
    for d in datas:
        if not isinstance(d, (bytes, bytearray, memoryview)):
            raise TypeError("%s: bytes or a list of bytes expected (got %s)" % (what, type(d).__name__))
    return single, datas


def _gpu_device(device, what):
    """`device` (None: the current one) as torch.device('cuda', index)"""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise _lib.CsmError("%s: the device must be a GPU (got %s); libcsm355 has no CPU path" % (what, dev))
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def _budget_chunks(own, budget):
    """(i, k) for runs of k consecutive items from i whose sizes own[i] ... sum to at most `budget`; one item is always taken"""
    i = 0
    while i < len(own):
        k, total = 1, own[i]
        while i + k < len(own) and total + own[i + k] <= budget:
            total += own[i + k]
            k += 1
        yield i, k
        i += k


def _check_sides(what, H, W):
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("%s: H and W must be in [1, 65535] (got %dx%d)" % (what, H, W))


def _image_batch(frames, what, size_check):
    """The acceptance rule of png_streams and the GIF route: device uint8 [n,H,W], [H,W] (grey), [n,H,W,3], [H,W,3] (colour; a
    uint8 tensor of rank 3 whose last dimension is 3 is one colour image) or bool [n,H,W], [H,W] (masks).  Returns (contiguous
    uint8 tensor [n,H,W] or [n,H,W,3], colour, mask); size_check(H, W, channels) runs before the device is looked at."""
    if not isinstance(frames, torch.Tensor):
        raise _lib.CsmError("%s: frames must be a device tensor (got %s)" % (what, type(frames).__name__))
    shape, mask = tuple(frames.shape), frames.dtype == torch.bool
    if mask:
        ok, colour = frames.dim() in (2, 3), False
    else:
        colour = frames.dim() == 4 or (frames.dim() == 3 and shape[-1] == 3)
        ok = frames.dtype == torch.uint8 and (frames.dim() in (2, 3) or (frames.dim() == 4 and shape[-1] == 3))
    if not ok:
        raise _lib.CsmError("%s: uint8 [n,H,W], [H,W], [n,H,W,3], [H,W,3] or bool [n,H,W], [H,W] expected (got %s %s)"
                            % (what, frames.dtype, shape))
    lead = 0 if frames.dim() == (3 if colour else 2) else 1
    size_check(int(shape[lead]), int(shape[lead + 1]), 3 if colour else 1)
    if not frames.is_cuda:
        raise _lib.CsmError("%s: frames must be a device tensor; libcsm355 has no CPU path" % what)
    im = frames.contiguous()
    im = im.view(torch.uint8) if mask else im
    return (im if lead else im.unsqueeze(0)), colour, mask


def _bgr_frames(frames, what, size_check):
    """The acceptance rule of jpeg_encode and webp_streams: device uint8 frames [n,H,W,3] or one [H,W,3], returned contiguous as
    [n,H,W,3]; size_check(H, W) runs before the device is looked at."""
    if not isinstance(frames, torch.Tensor):
        raise _lib.CsmError("%s: frames must be a device tensor (got %s)" % (what, type(frames).__name__))
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise _lib.CsmError("%s: uint8 frames [n,H,W,3] or [H,W,3] expected (got %s %s)" % (what, frames.dtype, tuple(frames.shape)))
    size_check(*(int(v) for v in frames.shape[-3:-1]))
    if not frames.is_cuda:
        raise _lib.CsmError("%s: frames must be a device tensor; libcsm355 has no CPU path" % what)
    fr = frames.contiguous()
    return fr.unsqueeze(0) if fr.dim() == 3 else fr


def _decode_groups(what, call, datas, infos, dev, budget, channels, layout, scratch_fn, decode_fn, info_per_file=False):
    """The chunked-call driver of the decoders: files (datas[i], infos[i]) go to the native decoder in groups of consecutive files
    whose scratch stays below `budget` (one file is always taken).  The format supplies
      layout(part, out_off) -> (blob bytes, descriptor tables, fill): for the files `part` = [(data, info)], whose pixels begin at
        out_off[j] of the group's output, the size of the blob to upload, the host int32 tables the native calls take (in their
        order; each is passed as pointer, rows) and fill(blob_h), which writes the blob; layout is also called for each file
        alone, to size that file's scratch, so everything costly belongs in fill;
      scratch_fn(*tables) and decode_fn(blob, blob bytes, *tables, out, out bytes, scratch, info_host, stream): the native pair.
    Yields (i, k, info_h, tensors) per group: its first file and file count, the ints the native call returned (one per file with
    info_per_file, else 4) and the files' [H,W,channels] tensors, views of one allocation."""
    import ctypes
    c_desc = ctypes.POINTER(ctypes.c_int32)

    def args(tables):
        return [a for t in tables for a in (t.ctypes.data_as(c_desc), i32(t.shape[0]))]

    own = [scratch_fn(*args(layout([item], [0])[1])) for item in zip(datas, infos)]
    for i, k in _budget_chunks(own, budget):
        part = list(zip(datas[i:i + k], infos[i:i + k]))
        out_off, oo = [], 0                                  # every file's pixels begin on a 16-byte boundary of one allocation
        for _, info in part:
            out_off.append(oo)
            oo += (info['height'] * info['width'] * channels + 15) & ~15
        blob_bytes, tables, fill = layout(part, out_off)     # `tables` named: alive while table_args points into them
        table_args = args(tables)
        blob_h = _np.zeros(blob_bytes, _np.uint8)
        fill(blob_h)
        with torch.cuda.device(dev):
            blob = torch.from_numpy(blob_h).to(dev)
            pixels = torch.empty(oo, dtype=torch.uint8, device=dev)
            need = scratch_fn(*table_args)
            if need == 0:
                raise _lib.CsmError("%s: %s" % (what, _lib.load().csm_last_error().decode()))
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
            info_h = (ctypes.c_int * (k if info_per_file else 4))()
            check(decode_fn(ptr(blob), i64(blob.numel()), *table_args, ptr(pixels), i64(oo), ptr(scratch), info_h, stream_ptr(dev)),
                  call)
        yield i, k, info_h, [pixels[o:o + info['height'] * info['width'] * channels].view(info['height'], info['width'], channels)
                             for o, (_, info) in zip(out_off, part)]


# ---- baseline JPEG of device frames (csrc/mjpeg.hip; the frames of video.write_mjpeg_avi) ---------------------------------
JPEG_SCRATCH_BYTES = 64 << 20          # frames are encoded in chunks whose scratch stays below this (one frame is always taken)


def jpeg_encode(frames, quality=90, subsampling='420'):
    """Baseline JPEG (JFIF, Annex K tables, one restart interval per MCU row; contract DESIGN.md §4.6) of device uint8 frames
    [n,H,W,3] (or one [H,W,3]) in B, G, R order.  Returns a list of n `bytes`, each a complete JPEG file.  quality 1..100 scales
    the quantisation tables by the IJG rule; subsampling is '420' (the default) or '444'.  The streams are built on the device
    (csm_jpeg_measure / _write) in chunks of frames whose scratch stays below JPEG_SCRATCH_BYTES; per chunk the host reads the
    [k,2] size table once, then only the bytes."""
    if isinstance(quality, bool) or not isinstance(quality, (int, _np.integer)) or not 1 <= quality <= 100:
        raise ValueError("jpeg_encode: quality must be an integer in [1, 100] (got %r)" % (quality,))
    if subsampling not in ('420', '444'):
        raise ValueError("jpeg_encode: subsampling must be '420' or '444' (got %r)" % (subsampling,))
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
        raise _lib.CsmError("jpeg_encode: frames must be a device tensor; libcsm355 has no CPU path")
    # named: alive until the kernels that read it are enqueued
    fr = _bgr_frames(frames, "jpeg_encode", lambda H, W: _check_sides("jpeg_encode", H, W))
    n, H, W = (int(v) for v in fr.shape[:3])
    L, dev, st = _lib.load(), fr.device, stream_ptr(fr.device)
    q, sub = i32(int(quality)), i32(int(subsampling))
    per_frame = L.csm_jpeg_scratch_bytes(i32(1), i32(H), i32(W), sub)
    step = max(1, JPEG_SCRATCH_BYTES // per_frame)
    out = []
    for f0 in range(0, n, step):
        part = fr[f0:f0 + step]
        k = int(part.shape[0])
        info = torch.empty((k, 2), dtype=torch.int64, device=dev)
        scratch = torch.empty(L.csm_jpeg_scratch_bytes(i32(k), i32(H), i32(W), sub), dtype=torch.uint8, device=dev)
        check(L.csm_jpeg_measure(ptr(part), i32(k), i32(H), i32(W), q, sub, ptr(info), ptr(scratch), st), "jpeg_measure")
        info_h = info.cpu().numpy()                         # the one sync before the blob is sized
        total = int(info_h[-1, 0] + info_h[-1, 1])
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        check(L.csm_jpeg_write(i32(k), i32(H), i32(W), q, sub, ptr(info), ptr(blob), ptr(scratch), st), "jpeg_write")
        host = blob.cpu().numpy().tobytes()
        out += [host[o:o + b] for o, b in info_h.tolist()]
    return out


# ---- baseline JPEG files to device frames (csrc/jpegdec.hip + jpegcode.py; utils.io_utils.imread_device) -------------------
JPEG_DECODE_SCRATCH_BYTES = 64 << 20   # files are decoded in chunks whose scratch stays below this (one file is always taken)


def jpeg_decode(files, device=None, stats=None, _infos=None, progressive=False):
    """Baseline JPEG files (contract DESIGN.md §4.8) to device uint8 [H,W,3] tensors in B, G, R order.  `files` is one `bytes` (one
    tensor is returned) or a list of `bytes` (a list is returned); sizes and modes (grey, 4:4:4, 4:2:2, 4:2:0, with or without
    restart markers) may differ within a call.  A grey file gives three equal channels.  EXIF orientation is NOT applied.  The
    host parses the markers (jpegcode.probe; a stream the decoder does not take raises jpegcode.Unsupported) and uploads only the
    files' entropy bytes and tables; Huffman decoding, the inverse DCT, chroma upsampling and colour conversion run on the device
    (csm_jpeg_decode) in chunks of files whose scratch stays below JPEG_DECODE_SCRATCH_BYTES.  Corrupt entropy data raises
    CsmError.  The tensors of a chunk are views of one allocation.  `stats` (a dict) receives 'passes': the synchronisation passes
    between workgroups of every chunk.

    progressive=True also takes progressive files (SOF2; jpegcode.probe(data, progressive=True) names the scan
    scripts that are taken), mixed with baseline files in any order: the baseline files of the call go through csm_jpeg_decode, the
    progressive ones through csm_jpeg_decode_progressive, each in chunks under the same budget, and the tensors come back in the
    order of `files`.  `stats` then also receives 'progressive' (the indices of the progressive files), 'levels' (the dependency
    levels launched for every progressive chunk) and 'progressive_passes'."""
    from . import jpegcode
    single, datas = _byte_files(files, "jpeg_decode")
    if _infos is not None:
        infos = _infos
    elif progressive:
        infos = [jpegcode.probe(d, progressive=True) for d in datas]
    else:
        infos = [jpegcode.probe(d) for d in datas]
    dev = _gpu_device(device, "jpeg_decode")
    L = _lib.load()
    prog = [i for i, info in enumerate(infos) if info.get('progressive')]
    if prog and not progressive:
        raise jpegcode.Unsupported("progressive (SOF2)")
    base = [i for i in range(len(datas)) if not infos[i].get('progressive')]
    out = [None] * len(datas)
    passes = []
    if base:
        tensors, passes = _jpeg_decode_baseline(L, [datas[i] for i in base], [infos[i] for i in base], dev)
        for i, t in zip(base, tensors):
            out[i] = t
    if stats is not None:
        stats['passes'] = passes
    if progressive:
        levels, ppasses = [], []
        if prog:
            tensors, levels, ppasses = _jpeg_decode_progressive(L, [datas[i] for i in prog], [infos[i] for i in prog], dev)
            for i, t in zip(prog, tensors):
                out[i] = t
        if stats is not None:
            stats.update(progressive=prog, levels=levels, progressive_passes=ppasses)
    return out[0] if single else out


def _jpeg_decode_baseline(L, datas, infos, dev):
    from . import jpegcode
    words, tab = L.csm_jpeg_decode_desc_words(), jpegcode.FILE_TABLE_BYTES
    assert words == jpegcode.DESC_WORDS

    def layout(part, out_off):
        # the blob: every file's table region, then every file's entropy bytes, each on a 16-byte boundary
        ent_off, o = [], len(part) * tab
        for _, info in part:
            ent_off.append(o)
            o += (info['entropy'][1] - info['entropy'][0] + 15) & ~15
        desc = _np.zeros((len(part), words), _np.int32)
        for j, (_, info) in enumerate(part):
            desc[j] = jpegcode.descriptor(info, ent_off[j], j * tab, out_off[j])

        def fill(blob_h):
            for j, (d, info) in enumerate(part):
                blob_h[j * tab:(j + 1) * tab] = jpegcode.file_tables(info)
                s, e = info['entropy']
                blob_h[ent_off[j]:ent_off[j] + e - s] = _np.frombuffer(d, _np.uint8, e - s, s)
        return max(o, 16), (desc,), fill

    out, passes = [], []
    for _, _, info_h, tensors in _decode_groups("jpeg_decode", "jpeg_decode", datas, infos, dev, JPEG_DECODE_SCRATCH_BYTES, 3, layout,
                                                L.csm_jpeg_decode_scratch_bytes, L.csm_jpeg_decode):
        passes.append(int(info_h[0]))
        out += tensors
    return out, passes


def _jpeg_decode_progressive(L, datas, infos, dev):
    """the progressive files of jpeg_decode: (tensors, levels per chunk, synchronisation passes per chunk)"""
    from . import jpegcode
    words, swords, tab = L.csm_jpeg_decode_desc_words(), L.csm_jpeg_decode_scan_desc_words(), jpegcode.FILE_TABLE_BYTES
    assert words == jpegcode.DESC_WORDS and swords == jpegcode.SCAN_DESC_WORDS
    a16 = lambda v: (v + 15) & ~15

    def layout(part, out_off):
        """the blob of a chunk: every file's table region (its quantisation tables), then per scan its decode tables, its entropy
        bytes and, for a refinement with restart markers, where its intervals begin, each on a 16-byte boundary"""
        o = len(part) * tab
        pieces, rows = [], []
        desc = _np.zeros((len(part), words), _np.int32)
        for j, (d, info) in enumerate(part):
            head = dict(info, restart_interval=0, components=[dict(c, td=0, ta=0) for c in info['components']], huffman={}, entropy=(0, 0))
            desc[j] = jpegcode.descriptor(head, 0, j * tab, out_off[j])
            level_of = {s: lv for lv, ss in enumerate(jpegcode.scan_levels(info)) for s in ss}
            tabs = jpegcode.scan_tables(info)
            for si, sc in enumerate(info['scans']):
                tab_off = o
                if tabs[si].size:
                    pieces.append((o, tabs[si]))
                    o += a16(tabs[si].size)
                s, e = sc['entropy']
                ent_off = o
                pieces.append((o, _np.frombuffer(d, _np.uint8, e - s, s)))
                o += a16(e - s)
                iv_off = 0
                blocks, unit = jpegcode.scan_block_count(info, sc)
                per = sc['restart_interval'] * unit
                if sc['ah'] and per and blocks > per:
                    want = -(-blocks // per)
                    iv = jpegcode.scan_intervals(d, sc)[:want]
                    iv = _np.concatenate([iv, _np.full(want - iv.size, e - s, _np.int32)])      # a missing marker: no data
                    iv_off = o
                    pieces.append((o, iv.view(_np.uint8)))
                    o += a16(iv.size * 4)
                rows.append(jpegcode.scan_descriptor(info, si, j, ent_off, tab_off, level_of[si], iv_off))

        def fill(blob_h):
            for j, (_, info) in enumerate(part):
                blob_h[j * tab:(j + 1) * tab] = quant_only(info)
            for at, arr in pieces:
                blob_h[at:at + arr.size] = arr
        return max(o, 16), (desc, _np.stack(rows)), fill

    def quant_only(info):
        t = _np.zeros(tab, _np.uint8)
        q = _np.zeros((3, 64), _np.uint16)
        for i, c in enumerate(info['components']):
            q[i, list(jpegcode.ZIGZAG)] = info['qtables'][c['tq']]
        t[jpegcode.HUFF_SLOTS * jpegcode.TABLE_BYTES:] = q.view(_np.uint8).ravel()
        return t

    out, levels, passes = [], [], []
    for _, _, info_h, tensors in _decode_groups("jpeg_decode", "jpeg_decode_progressive", datas, infos, dev, JPEG_DECODE_SCRATCH_BYTES, 3,
                                                layout, L.csm_jpeg_decode_progressive_scratch_bytes, L.csm_jpeg_decode_progressive):
        passes.append(int(info_h[0]))
        levels.append(int(info_h[1]))
        out += tensors
    return out, levels, passes


# ---- PNG files to device frames (csrc/pngdec.hip + pngread.py; utils.io_utils.imread_device) ------------------------------------
PNG_DECODE_SCRATCH_BYTES = 512 << 20   # files are decoded in chunks whose scratch stays below this (one file is always taken)


def png_decode(files, device=None, stats=None, _infos=None):
    """PNG files (contract DESIGN.md §4.9) to device uint8 [H,W,3] tensors in B, G, R order, equal to utils.io_utils.imread on every
    byte.  `files` is one `bytes` (one tensor is returned) or a list of `bytes` (a list is returned); sizes and colour types (grey,
    RGB, palette, grey + alpha, RGBA; 8 bits, not interlaced) may differ within a call.  Alpha is dropped, grey gives three equal
    channels.  The host walks the chunks (pngread.probe; a file the decoder does not take raises pngread.Unsupported) and uploads
    only the IDAT payloads and the palettes; inflate, the unfiltering and the colour conversion run on the device
    (csm_png_decode) in chunks of files whose scratch stays below PNG_DECODE_SCRATCH_BYTES.  A corrupt stream (invalid deflate
    data, a wrong Adler-32, a filter type above 4) raises CsmError.  The tensors of a chunk are views of one allocation.  `stats`
    (a dict) receives 'rounds': per chunk, the pointer-doubling rounds (launched, that did work)."""
    from . import pngread
    single, datas = _byte_files(files, "png_decode")
    infos = _infos if _infos is not None else [pngread.probe(d) for d in datas]
    dev = _gpu_device(device, "png_decode")
    L = _lib.load()
    words = L.csm_png_decode_desc_words()
    assert words == pngread.DESC_WORDS

    def layout(part, out_off):
        # the blob: every file's palette (768 bytes), then every file's zlib stream, each on a 16-byte boundary and padded to one
        stream_off, o = [], len(part) * 768
        for _, info in part:
            stream_off.append(o)
            o += (info['stream_bytes'] + 15) & ~15
        desc = _np.zeros((len(part), words), _np.int32)
        for j, (_, info) in enumerate(part):
            desc[j] = pngread.descriptor(info, stream_off[j], j * 768, out_off[j])

        def fill(blob_h):
            for j, (d, info) in enumerate(part):
                blob_h[j * 768:(j + 1) * 768] = info['palette'].reshape(-1)
                blob_h[stream_off[j]:stream_off[j] + info['stream_bytes']] = pngread.zlib_stream(d, info)
        return o, (desc,), fill

    out, rounds = [], []
    for _, _, info_h, tensors in _decode_groups("png_decode", "png_decode", datas, infos, dev, PNG_DECODE_SCRATCH_BYTES, 3, layout,
                                                L.csm_png_decode_scratch_bytes, L.csm_png_decode):
        rounds.append((int(info_h[0]), int(info_h[1])))
        out += tensors
    if stats is not None:
        stats['rounds'] = rounds
    return out[0] if single else out


# ---- GIF files to device frames (csrc/gifdec.hip + gifread.py; video.read_gif) ---------------------------------------------------
# The LZW stage takes 5 B of scratch per pixel of the images of one native call (4 B source position + 1 B literal, DESIGN.md
# §4.17), and every image is walked by one wave: 512 MiB hold about a hundred 1024 x 1024 frames, enough waves to spread over the CUs.
GIF_DECODE_SCRATCH_BYTES = 512 << 20   # images are decoded in groups whose scratch stays below this (one image is always taken)
_GIF_GROUP_IMAGES = 65535              # images of one native call at the most


def gif_decode(files, device=None, alpha=False, stats=None, _infos=None):
    """GIF files (GIF87a / GIF89a; contract DESIGN.md §4.17) to device uint8 tensors, one [n,H,W,3] in B, G, R order per file (n its
    frames, H x W its logical screen), equal on every byte to what Pillow shows after seek(i) and convert('RGB'); with alpha=True
    [n,H,W,4] in B, G, R, A order, equal to convert('RGBA').  `files` is one `bytes` (one tensor is returned) or a list of `bytes`
    (a list is returned); sizes and frame counts may differ within a call.  The host walks the container (gifread.probe; a file the
    decoder does not take raises gifread.Unsupported), joins every image's data sub-blocks and uploads only those compressed bytes
    and the colour tables; LZW decoding, interlace, transparency, the colour tables and the disposal methods run on the device
    (csm_gif_decode).  The LZW stage works on groups of consecutive images whose scratch stays below GIF_DECODE_SCRATCH_BYTES, one
    native call per group, so a clip larger than the budget still decodes; only the images' indices (1 byte per pixel) stay until
    the last call composes the frames, and the result does not depend on the budget.  Corrupt LZW data raises CsmError.  The
    tensors of a call are views of one allocation.  `stats` (a dict) receives 'groups' (the images of every native call) and
    'rounds' (per native call the pointer-doubling rounds launched and the rounds that did work)."""
    import ctypes
    from . import gifread
    single, datas = _byte_files(files, "gif_decode")
    infos = _infos if _infos is not None else [gifread.probe(d) for d in datas]
    dev = _gpu_device(device, "gif_decode")
    L = _lib.load()
    words = L.csm_gif_decode_desc_words()
    assert words == gifread.DESC_WORDS == gifread.FILE_WORDS
    channels = 4 if alpha else 3
    a16 = lambda v: (v + 15) & ~15
    # the blob: per file its global table, per image with one its local table (768 bytes each, zero-padded), then every image's
    # LZW bytes, each on a 16-byte boundary and padded to one
    rows, frows, tables, streams, own = [], [], [], [], []
    o, idx_off, out_off = 0, 0, 0
    shapes = []
    for j, (d, info) in enumerate(zip(datas, infos)):
        frows.append(gifread.file_descriptor(info, len(rows), out_off, channels))
        n, H, W = len(info['frames']), info['height'], info['width']
        shapes.append((out_off, n, H, W))
        out_off += a16(n * H * W * channels)
        gpal = None
        if info['global_palette'] is not None:
            gpal = o
            tables.append((o, info['global_palette']))
            o += 768
        for fr in info['frames']:
            pal_off = gpal
            if fr['palette'] is not None:
                pal_off = o
                tables.append((o, fr['palette']))
                o += 768
            rows.append([fr, j, d, pal_off, len(gifread.palette_of(info, fr)) // 3, idx_off])
            npix = fr['height'] * fr['width']
            idx_off += a16(npix)
            own.append(a16(npix) + a16(4 * npix))
    for r in rows:
        r.append(o)
        o += a16(r[0]['stream_bytes'])
    blob_h = _np.zeros(max(o, 16), _np.uint8)
    for at, t in tables:
        blob_h[at:at + len(t)] = _np.frombuffer(t, _np.uint8)
    desc = _np.zeros((len(rows), words), _np.int32)
    for i, (fr, j, d, pal_off, entries, ioff, soff) in enumerate(rows):
        blob_h[soff:soff + fr['stream_bytes']] = gifread.lzw_stream(d, fr)
        desc[i] = gifread.image_descriptor(fr, j, soff, pal_off, entries, ioff)
    fdesc = _np.stack(frows)
    c_desc = ctypes.POINTER(ctypes.c_int32)
    table_args = [desc.ctypes.data_as(c_desc), i32(desc.shape[0]), fdesc.ctypes.data_as(c_desc), i32(fdesc.shape[0])]
    groups = []
    for i, k in _budget_chunks(own, GIF_DECODE_SCRATCH_BYTES):
        groups += [(s, min(_GIF_GROUP_IMAGES, i + k - s)) for s in range(i, i + k, _GIF_GROUP_IMAGES)]
    rounds = []
    with torch.cuda.device(dev):
        blob = torch.from_numpy(blob_h).to(dev)
        idx = torch.empty(idx_off, dtype=torch.uint8, device=dev)
        pixels = torch.empty(out_off, dtype=torch.uint8, device=dev)
        for gi, (first, count) in enumerate(groups):
            need = L.csm_gif_decode_scratch_bytes(*table_args, i32(first), i32(count))
            if need == 0:
                raise _lib.CsmError("gif_decode: %s" % L.csm_last_error().decode())
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
            last = gi == len(groups) - 1
            info_h = (ctypes.c_int * 4)()
            check(L.csm_gif_decode(ptr(blob), i64(blob.numel()), *table_args, i32(first), i32(count), ptr(idx), i64(idx_off),
                                   ptr(pixels) if last else ctypes.c_void_p(0), i64(out_off if last else 0), i32(channels), ptr(scratch),
                                   info_h, stream_ptr(dev)), "gif_decode")
            rounds.append((int(info_h[0]), int(info_h[1])))
    if stats is not None:
        stats['groups'] = [k for _, k in groups]
        stats['rounds'] = rounds
    out = [pixels[o:o + n * H * W * channels].view(n, H, W, channels) for o, n, H, W in shapes]
    return out[0] if single else out


# ---- WebP files to device frames (csrc/webpdec.hip, csrc/webplossy.hip + webpread.py; utils.io_utils.imread_device) ------------
WEBP_DECODE_SCRATCH_BYTES = 64 << 20   # files are decoded in chunks whose scratch stays below this (one file is always taken)
WEBP_LOSSY_DECODE_SCRATCH_BYTES = 64 << 20   # the same for the lossy files of a call, which go to native calls of their own


def _webp_layout(part, out_off, channels, words, lossy):
    """_decode_groups' layout of WebP files: every VP8L / VP8 payload, and behind them every ALPH chunk's bytes behind its first,
    on 16-byte boundaries of the blob"""
    from . import webpread
    blob_off, alph_off, o = [], [], 0
    for _, info in part:
        blob_off.append(o)
        o += (info['payload'][1] - info['payload'][0] + 15) & ~15
    for _, info in part:
        alph_off.append(o)
        if lossy and info['alph']:
            o += (info['alph'][1] - info['alph'][0] - 1 + 15) & ~15
    desc = _np.zeros((len(part), words), _np.int32)
    for j, (d, info) in enumerate(part):
        if lossy:
            head = d[info['alph'][0]] if info['alph'] else 0
            desc[j] = webpread.lossy_descriptor(info, blob_off[j], out_off[j], channels, head, alph_off[j])
        else:
            desc[j] = webpread.descriptor(info, blob_off[j], out_off[j], channels)

    def fill(blob_h):
        for j, (d, info) in enumerate(part):
            p = webpread.payload(d, info)
            blob_h[blob_off[j]:blob_off[j] + p.size] = p
            if lossy and info['alph']:
                s, e = info['alph']
                blob_h[alph_off[j]:alph_off[j] + e - s - 1] = _np.frombuffer(d, _np.uint8, e - s - 1, s + 1)
    return max(o, 16), (desc,), fill


def webp_decode(files, device=None, alpha=False, stats=None, _infos=None, lossy=False):
    """WebP files to device uint8 tensors: [H,W,3] in B, G, R order, equal to utils.io_utils.imread on every byte, or with
    alpha=True [H,W,4] in B, G, R, A order, equal to PIL's convert('RGBA') (a file without alpha gets A = 255).  `files` is one
    `bytes` (one tensor is returned) or a list of `bytes` (a list is returned); sizes and features may differ within a call.
    Lossless files (VP8L; contract DESIGN.md §4.15) are always taken; lossy=True also takes lossy files (a VP8 key frame with or
    without an ALPH chunk; §4.16), mixed with lossless ones in any order: each kind goes to its own native calls (csm_webp_decode,
    csm_webp_lossy_decode) in chunks of files whose scratch stays below WEBP_DECODE_SCRATCH_BYTES and
    WEBP_LOSSY_DECODE_SCRATCH_BYTES, and the results come back in input order.  The host walks the RIFF container
    (webpread.probe; a file the decoders do not take -- animated, rotated, without lossy=True lossy -- raises
    webpread.Unsupported) and uploads only the chunks' payloads; entropy decoding, reconstruction and the colour store run on the
    device.  A corrupt stream raises CsmError.  A valid file with more prefix-code groups than the cap (webpread.GROUP_CAP, or
    one per 4 x 4 pixels in a smaller image; for a lossy file: in its alpha plane's stream) raises webpread.Unsupported after
    the decode, with the indices of such files in its `files` attribute.  The tensors of a chunk are views of one allocation.
    `stats` (a dict) receives 'chunks': the number of files of every native call of the lossless decoder, and with lossy=True
    'chunks_lossy': the same for the lossy one."""
    from . import webpread
    single, datas = _byte_files(files, "webp_decode")
    infos = _infos if _infos is not None else [webpread.probe(d, lossy=True) if lossy else webpread.probe(d) for d in datas]
    dev = _gpu_device(device, "webp_decode")
    L = _lib.load()
    words = L.csm_webp_decode_desc_words()
    assert words == webpread.DESC_WORDS and L.csm_webp_lossy_decode_desc_words() == words
    channels = 4 if alpha else 3
    out, over, chunks = [None] * len(datas), [], {False: [], True: []}
    for kind in (False, True):
        which = [i for i, info in enumerate(infos) if (info.get('kind') == 'lossy') == kind]
        if not which:
            continue
        budget, scratch_fn, decode_fn, cap = ((WEBP_LOSSY_DECODE_SCRATCH_BYTES, L.csm_webp_lossy_decode_scratch_bytes,
                                               L.csm_webp_lossy_decode, webpread.LOSSY_ERR_CAP) if kind else
                                              (WEBP_DECODE_SCRATCH_BYTES, L.csm_webp_decode_scratch_bytes, L.csm_webp_decode,
                                               webpread.ERR_CAP))
        for i, k, info_h, tensors in _decode_groups("webp_decode", "webp_lossy_decode" if kind else "webp_decode",
                                                    [datas[i] for i in which], [infos[i] for i in which], dev, budget, channels,
                                                    lambda part, out_off: _webp_layout(part, out_off, channels, words, kind),
                                                    scratch_fn, decode_fn, info_per_file=True):
            over += [which[i + j] for j in range(k) if info_h[j] & cap]
            chunks[kind].append(k)
            for j, t in enumerate(tensors):
                out[which[i + j]] = t
    if stats is not None:
        stats['chunks'] = chunks[False]
        if lossy:
            stats['chunks_lossy'] = chunks[True]
    if over:
        over.sort()
        e = webpread.Unsupported("webp_decode: file(s) %s of the call hold more prefix-code groups than the decoder's cap (%d)"
                                 % (over, webpread.GROUP_CAP))
        e.files = tuple(over)
        raise e
    return out[0] if single else out


# ---- PNG of device images (csrc/png.hip + pngcode.py; utils.io_utils.imwrite, the mask PNGs, video.write_apng) -------------
PNG_SCRATCH_BYTES = 64 << 20           # images are encoded in chunks whose scratch stays below this (one image is always taken)


def png_streams(images, bgr=True):
    """The zlib streams of png_encode (one `bytes` per image: what a PNG's IDAT or an APNG's fdAT chunk holds) and the geometry:
    returns (streams, width, height, colour_type)."""
    if not (isinstance(images, torch.Tensor) and images.is_cuda):
        raise _lib.CsmError("png_encode: images must be a device tensor; libcsm355 has no CPU path")

    def size_check(H, W, C):
        if not (1 <= H <= 65535 and 1 <= W <= 65535) or H * (W * C + 1) >= 2 ** 31:
            raise ValueError("png_encode: H and W must be in [1, 65535] and H * (W * channels + 1) below 2^31 (got %dx%d)" % (H, W))

    im, colour, mask = _image_batch(images, "png_encode", size_check)    # im named: alive until the kernels that read it are enqueued
    n, H, W = (int(v) for v in im.shape[:3])
    C = 3 if colour else 1
    from . import pngcode
    L, dev, st = _lib.load(), im.device, stream_ptr(im.device)
    flags = i32((1 if colour and bgr else 0) | (2 if mask else 0))
    per_image = L.csm_png_scratch_bytes(i32(1), i32(H), i32(W), i32(C))
    step = max(1, min(PNG_SCRATCH_BYTES // per_image, (2 ** 24 - 1) // H))
    words = L.csm_png_table_words()
    out = []
    for f0 in range(0, n, step):
        part = im[f0:f0 + step]
        k = int(part.shape[0])
        table = torch.empty((k, 288), dtype=torch.int32, device=dev)
        scratch = torch.empty(L.csm_png_scratch_bytes(i32(k), i32(H), i32(W), i32(C)), dtype=torch.uint8, device=dev)
        check(L.csm_png_measure(ptr(part), i32(k), i32(H), i32(W), i32(C), flags, ptr(table), ptr(scratch), st), "png_measure")
        table_h = table.cpu().numpy().view(_np.uint32)      # the one sync: the histograms size every stream exactly
        rows, spans, total = _np.empty((k, words), _np.uint32), [], 0
        for j in range(k):
            code = pngcode.build_code(table_h[j, :286])
            rows[j] = pngcode.table_row(code, table_h[j, 286], total)
            spans.append((total, code['bytes']))
            total += (code['bytes'] + 3) & ~3
        host_table = torch.from_numpy(rows.view(_np.int32)).to(dev)
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        check(L.csm_png_write(i32(k), i32(H), i32(W), i32(C), ptr(host_table), ptr(blob), i64(total), ptr(scratch), st), "png_write")
        host = blob.cpu().numpy().tobytes()
        out += [host[o:o + b] for o, b in spans]
    return out, W, H, 2 if colour else 0


def png_encode(images, bgr=True):
    """PNG files (8 bit, no interlace, no alpha; contract DESIGN.md §4.7) of device images: uint8 [n,H,W] or [H,W] (grey, colour
    type 0), uint8 [n,H,W,3] or [H,W,3] (colour type 2; B, G, R in memory unless bgr=False, written R, G, B), or bool [n,H,W] /
    [H,W] masks (written as 0 / 255 grey).  A uint8 tensor of rank 3 whose last dimension is 3 is one colour image.  Returns a list
    of n `bytes`, each a complete, lossless PNG.  Filtering, the run parse, the histogram, the Adler-32 and the bit packing run on
    the device (csm_png_measure / _write) in chunks of images whose scratch stays below PNG_SCRATCH_BYTES; per chunk the host
    reads the [k,288] histogram table once, builds each image's Huffman code (pngcode.build_code), then reads only the
    compressed bytes."""
    from . import pngcode
    streams, W, H, colour_type = png_streams(images, bgr)
    return [pngcode.png_file(s, W, H, colour_type) for s in streams]


# ---- WebP of device frames (csrc/webp.hip + webpcode.py; video.write_webp, npyframes2video's .webp route) -------------------
WEBP_SCRATCH_BYTES = 512 << 20         # frames are coded in chunks whose scratch stays below this (one frame is always taken)


def webp_streams(frames, quality=90, method=0):
    """The VP8 key frame (contract DESIGN.md §4.12) of every frame of the device uint8 frames [n,H,W,3] (or one [H,W,3]) in B, G, R
    order, one `bytes` per frame: returns (streams, width, height).  quality 1..100 picks the frame's one quantiser index.  Colour
    conversion, prediction, transforms and the boolean coder run on the device (csm_webp_measure / _write) in chunks of frames whose
    scratch stays below WEBP_SCRATCH_BYTES; per chunk the host reads the size table once, then only the compressed bytes, and puts
    the frame header and the partition sizes around them (webpcode.vp8_frame).

    The format bounds what a frame may need, and only the coded sizes tell: the first partition (modes and skip flags, typically
    under 1 byte per macroblock, 6.2 at the very worst) must stay below 2^19 bytes and a token partition below 2^24.  Frames of
    1024 x 1024 at quality 90 stay below 1 % of either; a frame of several thousand pixels a side, or a very noisy one at a high
    quality, can exceed it and then raises ValueError after the chunk's measure call, before any bytes are copied.

    method 0 (the default) writes 16x16 luma prediction and the default coefficient probabilities.  method 1 (contract DESIGN.md
    §4.12b) adds B_PRED macroblocks -- ten 4x4 predictors, chosen against the 16x16 mode by an integer rate-distortion rule -- and
    per-frame probability updates: files about half the size at the same quality number, for more device time per frame (§4.12b
    has both measured).  A first partition of method 1 is larger (up to 103 bytes per macroblock at the very worst)."""
    from . import webpcode
    quality = webpcode.check_quality(quality, "webp_streams")
    method = webpcode.check_method(method, "webp_streams")
    # named: alive until the kernels that read it are enqueued
    fr = _bgr_frames(frames, "webp_streams", lambda H, W: webpcode.check_size(W, H, "webp_streams"))
    n, H, W = (int(v) for v in fr.shape[:3])
    L, dev, st = _lib.load(), fr.device, stream_ptr(fr.device)
    q, units, me = i32(quality), webpcode.partitions(H) + 1, i32(method)
    per_frame = L.csm_webp_scratch_bytes_m(i32(1), i32(H), i32(W), me)
    step = max(1, min(WEBP_SCRATCH_BYTES // per_frame, (2 ** 20 - 1) // units))
    out = []
    for f0 in range(0, n, step):
        part = fr[f0:f0 + step]
        k = int(part.shape[0])
        info = torch.empty((k * units + 1, 2), dtype=torch.int64, device=dev)
        scratch = torch.empty(L.csm_webp_scratch_bytes_m(i32(k), i32(H), i32(W), me), dtype=torch.uint8, device=dev)
        check(L.csm_webp_measure_m(ptr(part), i32(k), i32(H), i32(W), q, me, ptr(info), ptr(scratch), st), "webp_measure")
        info_h = info.cpu().numpy()                         # the one sync before the blob is sized
        status, total = int(info_h[-1, 0]), int(info_h[-1, 1])
        if status:
            raise _lib.CsmError("webp_streams: a partition met the end of its scratch segment (status %d)" % status)
        sizes = info_h[:-1, 1].reshape(k, units)            # refuse what the frame header cannot hold before the blob is made
        if int(sizes[:, 0].max()) >= webpcode.MAX_FIRST_BYTES or int(sizes[:, 1:].max()) >= webpcode.MAX_PART_BYTES:
            raise ValueError("webp_streams: a %dx%d frame at quality %d needs a first partition of %d bytes (limit %d) and a token "
                             "partition of %d (limit %d)" % (W, H, quality, int(sizes[:, 0].max()), webpcode.MAX_FIRST_BYTES - 1,
                                                             int(sizes[:, 1:].max()), webpcode.MAX_PART_BYTES - 1))
        blob = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        check(L.csm_webp_write_m(i32(k), i32(H), i32(W), me, ptr(blob), i64(total), ptr(scratch), st), "webp_write")
        host = blob.cpu().numpy().tobytes()
        pieces = [host[o:o + b] for o, b in info_h[:-1].tolist()]
        out += [webpcode.vp8_frame(pieces[j * units], pieces[j * units + 1:(j + 1) * units], W, H) for j in range(k)]
    return out, W, H


def webp_encode(frames, quality=90, method=0):
    """Still WebP files (lossy, one VP8 key frame each; contract DESIGN.md §4.12, method 1 §4.12b) of device uint8 frames [n,H,W,3]
    (or one [H,W,3]) in B, G, R order: a list of n `bytes`, each a complete .webp file (webp_streams, then webpcode.still_file)."""
    from . import webpcode
    return [webpcode.still_file(s) for s in webp_streams(frames, quality=quality, method=method)[0]]


# ---- lossless WebP of device images (csrc/webpll.hip + webpcode.py; the instance cut-outs, utils.io_utils.imwrite) ------------
WEBPLL_SCRATCH_BYTES = 256 << 20       # images are coded in chunks whose scratch stays below this (one image is always taken)


def _webpll_images(images):
    """the acceptance rule of webp_encode_lossless: a list of (contiguous uint8 tensor [H,W,C] or [H,W], H, W, C, mask)"""
    what = "webp_encode_lossless"
    if isinstance(images, torch.Tensor):
        if not images.is_cuda:
            raise _lib.CsmError("%s: images must be device tensors; libcsm355 has no CPU path" % what)
        if images.dtype == torch.bool:
            ok, batch = images.dim() in (2, 3), images.dim() == 3
        else:
            ok = images.dtype == torch.uint8 and (images.dim() in (2, 3) or (images.dim() == 4 and images.shape[-1] in (3, 4)))
            batch = images.dim() == 4 or (images.dim() == 3 and images.shape[-1] not in (3, 4))
        if not ok:
            raise _lib.CsmError("%s: uint8 [n,H,W,4], [n,H,W,3], [n,H,W], one such image, bool [n,H,W] or [H,W], or a list of "
                                "images expected (got %s %s)" % (what, images.dtype, tuple(images.shape)))
        items = list(images.unbind(0)) if batch else [images]
    elif isinstance(images, (list, tuple)):
        items = list(images)
    else:
        raise _lib.CsmError("%s: a device tensor or a list of device tensors expected (got %s)" % (what, type(images).__name__))
    out = []
    for im in items:
        if not isinstance(im, torch.Tensor) or not im.is_cuda:
            raise _lib.CsmError("%s: images must be device tensors; libcsm355 has no CPU path" % what)
        mask = im.dtype == torch.bool
        if not ((mask and im.dim() == 2) or (im.dtype == torch.uint8 and (im.dim() == 2 or (im.dim() == 3 and im.shape[-1] in (3, 4))))):
            raise _lib.CsmError("%s: every image must be uint8 [H,W], [H,W,3], [H,W,4] or bool [H,W] (got %s %s)"
                                % (what, im.dtype, tuple(im.shape)))
        H, W = int(im.shape[0]), int(im.shape[1])
        if not (1 <= H <= 16384 and 1 <= W <= 16384):
            raise ValueError("%s: H and W must be in [1, 16384] (got %dx%d)" % (what, H, W))
        im = im.contiguous()
        out.append((im.view(torch.uint8) if mask else im, H, W, int(im.shape[2]) if im.dim() == 3 else 1, mask))
    if out and any(t[0].device != out[0][0].device for t in out):
        raise _lib.CsmError("%s: the images must lie on one device" % what)
    return out


def webp_encode_lossless(images):
    """Lossless WebP files (VP8L; contract DESIGN.md §4.13) of device images: uint8 [n,H,W,4] (B, G, R, A in memory; the file
    carries the alpha), [n,H,W,3] (B, G, R), [n,H,W] (grey), bool [n,H,W] masks (written 0 / 255), one such image without the
    leading n (a uint8 tensor of rank 3 whose last dimension is 3 or 4 is one colour image), or a LIST of [H,W] / [H,W,C] tensors
    of mixed sizes and channel counts.  Returns a list of `bytes`, each a complete .webp file that decodes to the input bit for
    bit; an empty batch or list gives [].  Subtract-green, the predictor choice, the run parse, the histograms and the bit packing
    run on the device (csm_webpll_measure / _write), a whole list in one call through a per-image descriptor table, in chunks of
    images whose scratch stays below WEBPLL_SCRATCH_BYTES; per chunk the host reads the [2k,1088] histogram table once, builds
    the prefix codes and every header bit (webpcode.ll_image_code), then reads only the compressed bytes."""
    import ctypes
    from . import webpcode
    items = _webpll_images(images)
    if not items:
        return []
    L, dev = _lib.load(), items[0][0].device
    st = stream_ptr(dev)
    words, mwords, twords = L.csm_webpll_desc_words(), L.csm_webpll_measure_words(), L.csm_webpll_table_words()
    assert (words, mwords, twords) == (8, webpcode.LL_SYMS, webpcode.LL_TABLE_WORDS)
    c_desc = ctypes.POINTER(ctypes.c_int64)

    def descriptors(part):
        desc = _np.zeros((len(part), words), _np.int64)
        for j, (im, H, W, C, mask) in enumerate(part):
            desc[j, :4] = (im.data_ptr(), H, W, C | (256 if mask else 0))
        need = L.csm_webpll_plan(desc.ctypes.data_as(c_desc), i32(len(part)))
        if not need:
            raise _lib.CsmError("webp_encode_lossless: the library refused the descriptors of %d images" % len(part))
        return desc, need

    own = [descriptors([it])[1] for it in items]
    out = []
    for i, k in _budget_chunks(own, WEBPLL_SCRATCH_BYTES):
        part = items[i:i + k]
        desc, need = descriptors(part)
        desc_h = desc.ctypes.data_as(c_desc)
        desc_d = torch.from_numpy(desc).to(dev)
        table = torch.empty((2 * k, mwords), dtype=torch.int32, device=dev)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        check(L.csm_webpll_measure(desc_h, ptr(desc_d), i32(k), ptr(table), ptr(scratch), st), "webpll_measure")
        table_h = table.cpu().numpy().view(_np.uint32)      # the one sync: the histograms size every stream exactly
        rows, spans, total = _np.empty((2 * k, twords), _np.uint32), [], 0
        for j, (im, H, W, C, mask) in enumerate(part):
            code = webpcode.ll_image_code(table_h[2 * j], table_h[2 * j + 1], W, H, C == 4)
            rows[2 * j] = webpcode.ll_table_row(code['planes'][0], total, code['bytes'])
            rows[2 * j + 1] = webpcode.ll_table_row(code['planes'][1], total, code['bytes'])
            spans.append((total, code['bytes']))
            total += (code['bytes'] + 3) & ~3
        host_table = torch.from_numpy(rows.view(_np.int32)).to(dev)
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        check(L.csm_webpll_write(desc_h, ptr(desc_d), i32(k), ptr(host_table), ptr(blob), i64(total), ptr(scratch), st), "webpll_write")
        host = blob.cpu().numpy().tobytes()
        out += [webpcode.lossless_file(host[o:o + b]) for o, b in spans]
    return out


# ---- instance cut-outs with transparency (csrc/cutout.hip) --------------------------------------------------------------------
def _cutout_masks(masks, what):
    if not (isinstance(masks, torch.Tensor) and masks.is_cuda):
        raise _lib.CsmError("%s: masks must be a device tensor; libcsm355 has no CPU path" % what)
    if masks.dtype not in (torch.uint8, torch.bool) or masks.dim() != 3:
        raise _lib.CsmError("%s: uint8 or bool masks [n,H,W] expected (got %s %s)" % (what, masks.dtype, tuple(masks.shape)))
    m = masks.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def mask_bboxes(masks):
    """The tight boxes of device masks uint8 / bool [n,H,W]: a device int32 [n,4] = x0, y0, x1, y1, end-exclusive; an empty mask
    gives 0, 0, 0, 0 (csm_mask_bbox: one launch for any n)."""
    m = _cutout_masks(masks, "mask_bboxes")
    n, H, W = (int(v) for v in m.shape)
    boxes = torch.empty((n, 4), dtype=torch.int32, device=m.device)
    if n and (H < 1 or W < 1):
        raise _lib.CsmError("mask_bboxes: empty mask planes (got %s)" % (tuple(m.shape),))
    if n:
        check(_lib.load().csm_mask_bbox(ptr(m), i32(n), i32(H), i32(W), ptr(boxes), stream_ptr(m.device)), "mask_bbox")
    return boxes


def cutout_bgra(img, masks, alpha=None, pad=0, indices=None):
    """Instance cut-outs with transparency: for every mask (or those of `indices`) the frame's pixels inside the mask's tight box,
    grown by `pad` >= 0 and clipped to the frame, as a device uint8 [h,w,4] image B, G, R, A.  A is 255 where the mask is set, or
    with a float32 alpha plane [H,W] (uint8)(clamp(alpha, 0, 1) * 255), truncated, where the mask is set; 0 elsewhere, and colour
    is zero wherever A is 0.  img: device uint8 [H,W,3] (B, G, R); masks: device uint8 / bool [n,Hm,Wm], the frame's size or up to
    2 px smaller (the overlap is used).  Returns a list of views of ONE packed buffer, None at the place of an empty mask.  The
    only readback is the [n,4] box table, which sizes the buffer; every instance is composed in one launch (csm_cutout_bgra)."""
    import ctypes
    what = "cutout_bgra"
    if not (isinstance(img, torch.Tensor) and img.is_cuda):
        raise _lib.CsmError("%s: img must be a device tensor; libcsm355 has no CPU path" % what)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[-1] != 3:
        raise _lib.CsmError("%s: a uint8 frame [H,W,3] expected (got %s %s)" % (what, img.dtype, tuple(img.shape)))
    m = _cutout_masks(masks, what)
    H, W = int(img.shape[0]), int(img.shape[1])
    n, Hm, Wm = (int(v) for v in m.shape)
    if not (0 <= H - Hm <= 2 and 0 <= W - Wm <= 2) or Hm < 1 or Wm < 1:
        raise _lib.CsmError("%s: masks of %dx%d do not fit a frame of %dx%d (the same size or up to 2 px smaller)" % (what, Hm, Wm, H, W))
    if isinstance(pad, bool) or int(pad) != pad or pad < 0:
        raise ValueError("%s: pad must be an integer >= 0 (got %r)" % (what, pad))
    pad = int(pad)
    if alpha is not None:
        if not (isinstance(alpha, torch.Tensor) and alpha.is_cuda and alpha.dtype == torch.float32 and tuple(alpha.shape) == (H, W)):
            raise _lib.CsmError("%s: alpha must be a device float32 plane [%d,%d]" % (what, H, W))
        alpha = alpha.contiguous()
    idx = list(range(n)) if indices is None else [int(v) for v in indices]
    if any(not 0 <= v < n for v in idx):
        raise IndexError("%s: indices must lie in [0, %d)" % (what, n))
    if not idx:
        return []
    im = img.contiguous()
    L, dev, st = _lib.load(), im.device, stream_ptr(im.device)
    boxes = mask_bboxes(m).cpu().numpy()                    # the one readback: it sizes the buffer
    words = L.csm_cutout_job_words()
    jobs, shapes, total, pixels = [], [], 0, 0
    for v in idx:
        x0, y0, x1, y1 = (int(b) for b in boxes[v])
        if x1 <= x0 or y1 <= y0:
            shapes.append(None)
            continue
        x0, y0, x1, y1 = max(0, x0 - pad), max(0, y0 - pad), min(W, x1 + pad), min(H, y1 + pad)
        jobs.append((v, x0, y0, x1, y1, total, pixels, 0))
        shapes.append((total, y1 - y0, x1 - x0))
        pixels += (y1 - y0) * (x1 - x0)
        total = pixels * 4
    if not jobs:
        return [None] * len(idx)
    jobs_h = _np.array(jobs, _np.int64).reshape(-1, words)
    jobs_d = torch.from_numpy(jobs_h).to(dev)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    check(L.csm_cutout_bgra(ptr(im), i32(H), i32(W), ptr(m), i32(n), i32(Hm), i32(Wm), ptr(alpha),
                            jobs_h.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ptr(jobs_d), i32(len(jobs)), ptr(out), i64(total), st),
          "cutout_bgra")
    return [None if s is None else out[s[0]:s[0] + s[1] * s[2] * 4].view(s[1], s[2], 4) for s in shapes]


# ---- instance overlays (csrc/overlay.hip) ------------------------------------------------------------------------
def overlay_line_width(H, W):
    """the reference's box line width (anime_instances.py:166): max(round((H + W + 3) / 2 * 0.003), 2), Python's round"""
    return max(round((H + W + 3) / 2 * 0.003), 2)


def _per_frame(value, n, name):
    if value is None:
        return [None] * n
    if not isinstance(value, (list, tuple)) or len(value) != n:
        raise ValueError("draw_instances_many: %s must be None or a list with one entry per frame" % name)
    return list(value)


def draw_instances_many(frames, instances, colors=None, indices=None, draw_bbox=True, draw_ins_mask=True, draw_ins_contour=False,
                        mask_alpha=0.75, line_width=None):
    """ops.draw_instances for a list of frames, which may differ in size, in ONE native call (csm_draw_instances).  instances: per
    frame an object with .masks and .bboxes (AnimeInstances; masks None = no instance) or a (masks, bboxes) pair; colors and
    indices: None or a list with one entry (or None) per frame.  Returns a list of device uint8 [H,W,3] tensors."""
    import ctypes
    from .anime_instances import get_color
    what = "draw_instances"
    frames, instances = list(frames), list(instances)
    if len(frames) != len(instances):
        raise ValueError("%s: %d frames but %d sets of instances" % (what, len(frames), len(instances)))
    colors, indices = _per_frame(colors, len(frames), "colors"), _per_frame(indices, len(frames), "indices")
    if isinstance(mask_alpha, bool) or not 0.0 <= float(mask_alpha) <= 1.0:
        raise ValueError("%s: mask_alpha must lie in [0, 1] (got %r)" % (what, mask_alpha))
    if line_width is not None and (isinstance(line_width, bool) or int(line_width) != line_width or not 1 <= line_width < 1 << 30):
        raise ValueError("%s: line_width must be an integer >= 1 (got %r)" % (what, line_width))
    if not frames:
        return []
    L = _lib.load()
    words = L.csm_overlay_job_words()
    jobs_h = _np.zeros((len(frames), words), _np.int64)
    entries, cols, keep, outs = [], [], [], []
    for j, (frame, inst) in enumerate(zip(frames, instances)):
        im = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(_np.ascontiguousarray(frame))
        im = (im if im.is_cuda else im.cuda()).contiguous()
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[-1] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise _lib.CsmError("%s: a uint8 frame [H,W,3] expected (got %s %s)" % (what, im.dtype, tuple(im.shape)))
        H, W = int(im.shape[0]), int(im.shape[1])
        masks, boxes = (inst.masks, inst.bboxes) if hasattr(inst, 'masks') else inst
        n = 0 if masks is None else len(masks)
        m = b = None
        if n:
            m = masks if isinstance(masks, torch.Tensor) else torch.from_numpy(_np.ascontiguousarray(masks))
            if m.dtype not in (torch.uint8, torch.bool) or m.dim() != 3:
                raise _lib.CsmError("%s: uint8 or bool masks [n,H,W] expected (got %s %s)" % (what, m.dtype, tuple(m.shape)))
            if tuple(m.shape[1:]) != (H, W):
                raise ValueError("%s: masks of %dx%d over a frame of %dx%d: the reference's cv2.resize(INTER_AREA) of the frame to the "
                                 "masks' size (anime_instances.py:151-153) is not built; resize the instances to the frame"
                                 % (what, m.shape[1], m.shape[2], H, W))
            m = m.to(im.device).contiguous()
            m = m.view(torch.uint8) if m.dtype == torch.bool else m
            b = boxes if isinstance(boxes, torch.Tensor) else torch.from_numpy(_np.ascontiguousarray(boxes))
            if tuple(b.shape) != (n, 4) or b.dtype.is_floating_point or b.dtype == torch.bool:
                raise _lib.CsmError("%s: integer xywh boxes [%d,4] expected (got %s %s)" % (what, n, b.dtype, tuple(b.shape)))
            b = b.to(im.device, torch.int32).contiguous()
        idx = list(range(n)) if indices[j] is None else [int(v) for v in indices[j]]
        if any(not 0 <= v < n for v in idx):
            raise ValueError("%s: draw indices must lie in [0, %d) (got %r)" % (what, n, idx))
        if colors[j] is None:
            col = _np.array([get_color(v) for v in idx], _np.uint8).reshape(-1, 3)
        else:
            col = colors[j].cpu().numpy() if isinstance(colors[j], torch.Tensor) else _np.asarray(colors[j])
            if col.shape != (len(idx), 3) or col.dtype != _np.uint8:
                raise ValueError("%s: colors must be uint8 [%d,3], one B, G, R per draw-list entry (got %s %s)"
                                 % (what, len(idx), col.dtype, col.shape))
        out = torch.empty_like(im)
        jobs_h[j, :10] = (im.data_ptr(), out.data_ptr(), 0 if m is None else m.data_ptr(), 0 if b is None else b.data_ptr(), H, W, n,
                          len(idx), len(entries), overlay_line_width(H, W) if line_width is None else int(line_width))
        entries += idx
        cols.append(col)
        keep.append((im, m, b))
        outs.append(out)
    dev = keep[0][0].device
    if any(k[0].device != dev for k in keep):
        raise _lib.CsmError("%s: the frames of one call must be on one device" % what)
    i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    if not L.csm_overlay_plan(jobs_h.ctypes.data_as(i64p), i32(len(frames)), i32(len(entries))):
        raise _lib.CsmError("%s: csm_overlay_plan refused the job table" % what)
    flags = (1 if draw_bbox else 0) | (2 if draw_ins_mask else 0) | (4 if draw_ins_contour else 0)
    entries_h = _np.array(entries, _np.int32)
    alpha = _np.float32(mask_alpha)
    jobs_d = torch.from_numpy(jobs_h).to(dev)
    entries_d = torch.from_numpy(entries_h).to(dev) if entries else None
    cols_d = torch.from_numpy(_np.concatenate(cols)).to(dev) if entries else None
    check(L.csm_draw_instances(jobs_h.ctypes.data_as(i64p), ptr(jobs_d), i32(len(frames)), entries_h.ctypes.data_as(i32p), ptr(entries_d),
                               ptr(cols_d), i32(len(entries)), i32(flags), f32(float(alpha)), f32(float(_np.float32(1) - alpha)),
                               stream_ptr(dev)), what)
    return outs


def draw_instances(img, masks, bboxes, colors=None, indices=None, draw_bbox=True, draw_ins_mask=True, draw_ins_contour=False,
                   mask_alpha=0.75, line_width=None):
    """The reference's instance picture (AnimeInstances.draw_instances, anime_instances.py:131-194) drawn on the device, byte-exact
    to the contract of DESIGN.md §4.14: a device uint8 [H,W,3] copy of the B, G, R frame `img` (numpy, uploaded, or a device tensor)
    with, for the instances of `indices` (any order, repeats allowed; default all) in that order, first every box outline
    (`bboxes` int xywh [n,4]; a crisp band `line_width` px thick, default the reference's rule), then every mask (`masks` bool or
    0 / 1 uint8 [n,H,W]) blended in float32 as d = d * (1 - mask_alpha) + mask_alpha * colour and truncated, then, with
    draw_ins_contour, every mask's edge pixels in its colour.  colors: uint8 [k,3] B, G, R per draw-list entry (default
    get_color(instance index)).  Masks of another size than the frame and indices outside 0..n-1 raise ValueError."""
    return draw_instances_many([img], [(masks, bboxes)], colors=None if colors is None else [colors],
                               indices=None if indices is None else [indices], draw_bbox=draw_bbox, draw_ins_mask=draw_ins_mask,
                               draw_ins_contour=draw_ins_contour, mask_alpha=mask_alpha, line_width=line_width)[0]


# ---- GIF of device frames (csrc/gif.hip + gifcode.py; video.write_gif, npyframes2video's .gif route) ----------------------
GIF_SCRATCH_BYTES = 64 << 20           # frames are coded in chunks whose scratch stays below this (one frame is always taken)


def gif_quantize(frames, palette=None, dither='ordered', bgr=True):
    """Frames to palette indices (contract DESIGN.md §4.10): returns (indices, palette), indices device uint8 [n,H,W], palette host
    uint8 [256,3] in R, G, B order.  frames: device uint8 [n,H,W,3] or [H,W,3] (B, G, R in memory unless bgr=False), uint8 [n,H,W] or
    [H,W] (grey) or bool masks (0 / 255); grey and masks keep their bytes as indices into the grey palette, never dithered.  Colour:
    without `palette` one device pass fills the clip's cell table (csm_gif_histogram), the host reads it once (512 KB) and cuts ONE
    palette for all frames (gifcode.build_palette); then every pixel takes the nearest of the 256 entries (csm_gif_map), after the
    8x8 Bayer offset of dither='ordered' or as it is with dither='none'."""
    from . import gifcode
    if dither not in ('ordered', 'none'):
        raise ValueError("gif_quantize: dither must be 'ordered' or 'none' (got %r)" % (dither,))
    if palette is not None:
        palette = gifcode.check_palette(palette)
    im, colour, mask = _image_batch(frames, "gif_quantize", lambda H, W, C: _check_sides("gif_quantize", H, W))
    if not colour:
        return (im * 255 if mask else im), gifcode.grey_palette()
    n, H, W = (int(v) for v in im.shape[:3])
    L, dev, st = _lib.load(), im.device, stream_ptr(im.device)
    if palette is None:
        if n * H * W >= gifcode.MAX_PIXELS:
            raise ValueError("gif_quantize: a clip of %d pixels; the uint32 cell table takes fewer than 2^29" % (n * H * W))
        table = torch.empty((gifcode.CELLS, 4), dtype=torch.int32, device=dev)
        check(L.csm_gif_histogram(ptr(im), i64(n * H * W), i32(1 if bgr else 0), ptr(table), st), "gif_histogram")
        palette = gifcode.build_palette(table.cpu().numpy().view(_np.uint32))     # the one sync of the palette
    pal_d = torch.from_numpy(palette).to(dev)
    indices = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    flags = i32((1 if bgr else 0) | (2 if dither == 'ordered' else 0))
    check(L.csm_gif_map(ptr(im), i32(n), i32(H), i32(W), flags, ptr(pal_d), ptr(indices), st), "gif_map")
    return indices, palette


def gif_streams(indices):
    """The LZW data of a GIF's frames (minimum code size 8, not yet framed into sub-blocks; contract DESIGN.md §4.10), one `bytes`
    per frame of the device uint8 indices [n,H,W] or [H,W]: returns (streams, width, height).  Coding and bit packing run on the
    device (csm_gif_measure / _write) in chunks of frames whose scratch stays below GIF_SCRATCH_BYTES; per chunk the host reads the
    byte counts once, then only the compressed bytes."""
    if not isinstance(indices, torch.Tensor):
        raise _lib.CsmError("gif_streams: indices must be a device tensor (got %s)" % type(indices).__name__)
    if indices.dtype != torch.uint8 or indices.dim() not in (2, 3):
        raise _lib.CsmError("gif_streams: uint8 [n,H,W] or [H,W] indices expected (got %s %s)" % (indices.dtype, tuple(indices.shape)))
    H, W = (int(v) for v in indices.shape[-2:])
    _check_sides("gif_streams", H, W)
    if not indices.is_cuda:
        raise _lib.CsmError("gif_streams: indices must be a device tensor; libcsm355 has no CPU path")
    im = indices.contiguous()                                   # named: alive until the kernels that read it are enqueued
    im = im.unsqueeze(0) if im.dim() == 2 else im
    n = int(im.shape[0])
    L, dev, st = _lib.load(), im.device, stream_ptr(im.device)
    per_frame = L.csm_gif_scratch_bytes(i32(1), i32(H), i32(W))
    segments = -(-H * W // 3839)
    step = max(1, min(GIF_SCRATCH_BYTES // per_frame, (2 ** 24 - 1) // segments))
    out = []
    for f0 in range(0, n, step):
        part = im[f0:f0 + step]
        k = int(part.shape[0])
        scratch = torch.empty(L.csm_gif_scratch_bytes(i32(k), i32(H), i32(W)), dtype=torch.uint8, device=dev)
        counts = torch.empty(k, dtype=torch.int64, device=dev)
        check(L.csm_gif_measure(ptr(part), i32(k), i32(H), i32(W), ptr(counts), ptr(scratch), st), "gif_measure")
        counts_h = counts.cpu().numpy()                         # the one sync: the byte counts size the blob exactly
        padded = (counts_h + 3) & ~3
        offs = _np.concatenate([[0], _np.cumsum(padded)])
        total = int(offs[-1])
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        check(L.csm_gif_write(i32(k), i32(H), i32(W), ptr(blob), i64(total), ptr(scratch), st), "gif_write")
        host = blob.cpu().numpy().tobytes()
        out += [host[int(o):int(o) + int(b)] for o, b in zip(offs[:-1], counts_h)]
    return out, W, H


def gif_encode(frames, fps=25, loop=0, order=None, dither='ordered', palette=None, bgr=True):
    """A complete animated GIF (GIF89a; contract DESIGN.md §4.10) of device frames, as `bytes`: gif_quantize, gif_streams, then the
    host container (gifcode.gif_file: one global 256-colour table, every frame the full canvas for round(100 / fps) centiseconds,
    `loop` repetitions, 0 = for ever).  `order` lists the coded frame each output frame takes (default: each once, in order)."""
    from . import gifcode
    gifcode.delay_cs(fps)                                       # refuse before any device work
    indices, palette = gif_quantize(frames, palette=palette, dither=dither, bgr=bgr)
    streams, W, H = gif_streams(indices)
    return gifcode.gif_file(streams, W, H, palette, fps=fps, loop=loop, order=order)


# ---- PatchMatch inpainting (animeinsseg/inpainting/patch_match.py; kenburns_effect.py:497-503) ----------------------------
def patchmatch_inpaint(img, mask, global_mask=None, patch_size=15, seed=0):
    """PatchMatch inpainting of device uint8 [H,W,3] `img` where the device uint8 `mask` ([H,W] or [H,W,1]) is non-zero;
    `global_mask` (same shapes) marks pixels that never serve inside a source patch.  Returns a new device uint8 [H,W,3]: known
    pixels unchanged, holes filled by the coarse-to-fine EM of csrc/patchmatch.hip (contract DESIGN.md §4.5, deterministic for a
    given seed).  The host reads the per-level counts once, between csm_patchmatch_prepare and csm_patchmatch_run."""
    for name, t in (("img", img), ("mask", mask), ("global_mask", global_mask)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise _lib.CsmError("patchmatch_inpaint: %s must be a device tensor; libcsm355 has no CPU path" % name)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise _lib.CsmError("patchmatch_inpaint: img must be uint8 [H,W,3] (got %s %s)" % (img.dtype, tuple(img.shape)))
    H, W = int(img.shape[0]), int(img.shape[1])
    p = int(patch_size)
    if p < 3 or p > 15 or p % 2 == 0:
        raise ValueError("patchmatch_inpaint: patch_size must be odd and in [3, 15] (got %d)" % p)
    if H < p or W < p:
        raise ValueError("patchmatch_inpaint: image %dx%d is smaller than the patch size %d" % (H, W, p))

    def flat(m, name):
        if m is None:
            return None
        if m.dtype not in (torch.uint8, torch.bool) or tuple(m.shape) not in ((H, W), (H, W, 1)):
            raise _lib.CsmError("patchmatch_inpaint: %s must be uint8 [H,W] or [H,W,1] (got %s %s)" % (name, m.dtype, tuple(m.shape)))
        m = m.contiguous()
        return m.view(torch.uint8) if m.dtype == torch.bool else m
    import ctypes
    L = _lib.load()
    im, mk, gm = img.contiguous(), flat(mask, "mask"), flat(global_mask, "global_mask")   # named: alive until the kernels are enqueued
    dev = im.device
    n = L.csm_patchmatch_levels(i32(H), i32(W), i32(p))
    info = torch.empty((n, 4), dtype=torch.int32, device=dev)
    scratch = torch.empty(L.csm_patchmatch_scratch_bytes(i32(H), i32(W), i32(p)), dtype=torch.uint8, device=dev)
    st = stream_ptr(dev)
    check(L.csm_patchmatch_prepare(ptr(im), ptr(mk), ptr(gm), i32(H), i32(W), i32(p), ptr(info), ptr(scratch), st), "patchmatch_prepare")
    info_h = _np.ascontiguousarray(info.cpu().numpy())     # the one sync: the schedule
    if info_h[0, 0] == 0 or info_h[0, 1] == 0:             # no valid source, or nothing to fill
        return im.clone()
    levels = 1
    while levels < n and info_h[levels, 0] > 0:
        levels += 1
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    check(L.csm_patchmatch_run(i32(H), i32(W), i32(p), i32(levels), info_h.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                               ctypes.c_uint(int(seed) & 0xFFFFFFFF), ptr(out), ptr(scratch), st), "patchmatch_run")
    return out
