#!/usr/bin/env python3
"""Generate tests/golden/net_*.npz from the REFERENCE's own torch modules (build container only).

The reference files are imported by path (ref_loader.py); their parameters/buffers are filled with
cartoonsegmentation_amd.weights.synth_tensor(<reference parameter name>, ...) -- the same closed-form
weights the build's own lowering uses -- then the reference module runs on CPU (eval mode).
Stored: input, output.  No weights and no reference code travel.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE); sys.path.insert(0, ROOT)
import ref_loader  # noqa: E402
from cartoonsegmentation_amd.weights import synth_tensor  # noqa: E402

ref_loader.install_stubs()


def fill_synthetic(module, prefix):
    """assign every parameter / buffer of a reference nn.Module from synth_tensor(prefix+name)"""
    kinds = {}
    for mname, m in module.named_modules():
        pre = mname + '.' if mname else ''
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            kinds[pre + 'weight'] = 'conv_w'; kinds[pre + 'bias'] = 'conv_b'
        elif isinstance(m, torch.nn.BatchNorm2d):
            kinds[pre + 'weight'] = 'bn_gamma'; kinds[pre + 'bias'] = 'bn_beta'
            kinds[pre + 'running_mean'] = 'bn_mean'; kinds[pre + 'running_var'] = 'bn_var'
        elif isinstance(m, torch.nn.PReLU):
            kinds[pre + 'weight'] = 'prelu'
    sd = module.state_dict()
    for name, t in sd.items():
        if name.endswith('num_batches_tracked'):
            continue
        t.copy_(torch.from_numpy(synth_tensor(prefix + name, tuple(t.shape), kinds[name])))
    module.load_state_dict(sd)
    return module.eval()


def isnet_cases():
    ref_loader._bare("animeinsseg"); ref_loader._bare("animeinsseg.models"); ref_loader._bare("animeinsseg.models.animeseg_refine")
    m = ref_loader.load_by_path("animeinsseg.models.animeseg_refine.isnet", "animeinsseg/models/animeseg_refine/isnet.py")
    net = fill_synthetic(m.ISNetDIS(in_ch=4), 'isnet.')
    for tag, (h, w) in (('64x64', (64, 64)), ('90x74', (90, 74))):
        g = np.random.default_rng(100 + h)
        x = g.uniform(0, 1, (1, 4, h, w)).astype(np.float32)
        with torch.no_grad():
            d1 = net(torch.from_numpy(x))[0][0]           # animeinsseg/__init__.py:653 uses [0][0]
        np.savez_compressed(os.path.join(HERE, 'net_isnet_%s.npz' % tag), x=x, d1=d1.numpy())
        print('isnet', tag, float(d1.mean()), float(d1.std()))


def leres_cases():
    for n in ("depth_modules", "depth_modules.leres", "depth_modules.leres.leres"):
        ref_loader._bare(n)
    ref_loader.load_by_path("depth_modules.leres.leres.Resnet", "depth_modules/leres/leres/Resnet.py")
    ref_loader.load_by_path("depth_modules.leres.leres.Resnext_torch", "depth_modules/leres/leres/Resnext_torch.py")
    ref_loader.load_by_path("depth_modules.leres.leres.network_auxi", "depth_modules/leres/leres/network_auxi.py")
    ref_loader.load_by_path("depth_modules.leres.leres.net_tools", "depth_modules/leres/leres/net_tools.py")
    m = ref_loader.load_by_path("depth_modules.leres.leres.multi_depth_model_woauxi",
                                "depth_modules/leres/leres/multi_depth_model_woauxi.py")
    net = fill_synthetic(m.RelDepthModel(backbone='resnext101'), 'leres.')
    for tag, (h, w) in (('64x64', (64, 64)), ('96x64', (96, 64))):
        g = np.random.default_rng(200 + h)
        x = g.normal(0, 1, (1, 3, h, w)).astype(np.float32)
        with torch.no_grad():
            y = net.depth_model(torch.from_numpy(x))
        np.savez_compressed(os.path.join(HERE, 'net_leres_%s.npz' % tag), x=x, y=y.numpy())
        print('leres', tag, float(y.mean()), float(y.std()))


INPAINT_SIZES = ((32, 40), (35, 45), (36, 44), (33, 40), (27, 61))


def inpaint_case(H, W):
    """whole Inpaint.forward of the reference (incl. its render_pointcloud CUDA text through cuda_on_cpu.h) at H x W; the sizes
    other than 32x40 take the odd-size crops of pointcloud_inpainting.py:165-166, :178-179 at one or more joins"""
    mu, co, cu = ref_loader.load_warp_modules()
    m = ref_loader.load_by_path("anime_3dkenburns.models.pointcloud_inpainting", "anime_3dkenburns/models/pointcloud_inpainting.py")
    net = fill_synthetic(m.Inpaint(), 'inpaint.')
    g = np.random.default_rng(77)
    img = g.uniform(0, 1, (1, 3, H, W)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    disp = (10 + 8 * yy / H + 14.0 / (1.0 + np.exp(np.clip((np.hypot(xx - 18, yy - 14) - 8) / 0.75, -60, 60)))).astype(np.float32)[None, None]
    disp = disp / disp.max() * 40.0
    seg = (np.hypot(xx - 18, yy - 14) < 8).astype(np.float32)[None, None].repeat(3, 1)
    shift = np.array([2.5, -1.5, -3.0], np.float32).reshape(1, 3, 1)
    common = {'fltFocal': W / 2.0, 'fltBaseline': 40.0, 'intWidth': W, 'intHeight': H}
    with torch.no_grad():
        out = net(torch.from_numpy(img), torch.from_numpy(disp.astype(np.float32)), torch.from_numpy(shift), common, torch.from_numpy(seg))
    np.savez_compressed(os.path.join(HERE, 'net_inpaint_%dx%d.npz' % (H, W)), img=img, disp=disp.astype(np.float32), shift=shift, seg=seg,
                        existing=out['tenExisting'].numpy(), image=out['tenImage'].numpy(), disparity=out['tenDisparity'].numpy(),
                        segmasks=out['segmasks'].numpy())
    print('inpaint %dx%d' % (H, W), float(out['tenExisting'].mean()), float(out['tenImage'].mean()), float(out['tenDisparity'].mean()))


def refine_case():
    """Refine.forward of anime_3dkenburns/models/disparity_refinement.py:97-126 (the depth refinement of kenburns_effect.py:619-622):
    image at the frame size, disparity at a quarter of it (the reference's own usage: the estimator output is smaller than the frame)"""
    m = ref_loader.load_by_path("anime_3dkenburns.models.disparity_refinement", "anime_3dkenburns/models/disparity_refinement.py")
    net = fill_synthetic(m.Refine(), 'refine.')
    g = np.random.default_rng(5)
    img = g.uniform(0, 1, (1, 3, 48, 64)).astype(np.float32)
    dsp = g.uniform(1, 40, (1, 1, 12, 16)).astype(np.float32)
    with torch.no_grad():
        y = net(torch.from_numpy(img), torch.from_numpy(dsp))
    np.savez_compressed(os.path.join(HERE, 'net_refine_48x64.npz'), img=img, dsp=dsp, y=y.numpy())
    print('refine', float(y.mean()), float(y.std()))


def disparity_case():
    """Semantics (VGG19-BN slices) + Disparity GridNet of anime_3dkenburns/models/disparity_estimation.py.  torchvision is absent:
    `torchvision.models.vgg19_bn` is supplied with torchvision's published cfg 'E' + batch norm ([EXT]); which of its entries are
    used, the ceil-mode pools, the input flip / normalisation and the whole GridNet are the reference's own text."""
    import types
    nn = torch.nn

    def vgg19_bn(pretrained=False, **kw):
        layers, c = [], 3
        for v in [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M']:
            if v == 'M':
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(c, v, kernel_size=3, padding=1), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
                c = v
        return types.SimpleNamespace(features=nn.Sequential(*layers))
    sys.modules['torchvision.models'].vgg19_bn = vgg19_bn
    sys.modules['torchvision'].models = sys.modules['torchvision.models']
    ref_loader._bare("anime_3dkenburns"); ref_loader._bare("anime_3dkenburns.models")
    m = ref_loader.load_by_path("anime_3dkenburns.models.disparity_estimation", "anime_3dkenburns/models/disparity_estimation.py")
    sem = fill_synthetic(m.Semantics(), 'semantics.')
    dis = fill_synthetic(m.Disparity(), 'disparity.')
    for tag, (h, w) in (('96x64', (96, 64)), ('64x128', (64, 128)), ('72x88', (72, 88))):      # 72x88: odd rows AND odd columns on the way down
        g = np.random.default_rng(300 + h)
        x = g.uniform(0, 1, (1, 3, h, w)).astype(np.float32)
        with torch.no_grad():
            s_ = sem(torch.from_numpy(x))
            d = dis(torch.from_numpy(x), s_)
        np.savez_compressed(os.path.join(HERE, 'net_disparity_%s.npz' % tag), x=x, sem=s_.numpy(), disp=d.numpy())
        print('disparity', tag, tuple(s_.shape), float(s_.mean()), tuple(d.shape), float(d.mean()), float(d.std()))


def zoe_head_case():
    """ZoeDepth.forward (zoedepth_v1.py:124-202) with the shipped ZoeD_M12_N configuration (config_zoedepth.json), its layers loaded
    from the reference files, and a stand-in `core` that returns seeded feature maps of the shapes MidasCore documents
    (rel_depth [B,H,W]; out_conv [B,32,H,W]; bottleneck + r4..r1 [B,256,H/32..H/2]): the MiDaS backbone itself comes from torch.hub
    and is not vendored.  The class statement is executed from the file's text (ref_loader.extract_def)."""
    import itertools
    import json
    nn = torch.nn
    for n in ("depth_modules", "depth_modules.zoedepth", "depth_modules.zoedepth.models", "depth_modules.zoedepth.models.layers"):
        ref_loader._bare(n)
    L = "depth_modules/zoedepth/models/layers/"
    att = ref_loader.load_by_path("depth_modules.zoedepth.models.layers.attractor", L + "attractor.py")
    dist = ref_loader.load_by_path("depth_modules.zoedepth.models.layers.dist_layers", L + "dist_layers.py")
    lb = ref_loader.load_by_path("depth_modules.zoedepth.models.layers.localbins_layers", L + "localbins_layers.py")
    ns = dict(torch=torch, nn=nn, itertools=itertools, DepthModel=nn.Module, MidasCore=None, load_state_from_resource=None,
              AttractorLayer=att.AttractorLayer, AttractorLayerUnnormed=att.AttractorLayerUnnormed,
              ConditionalLogBinomial=dist.ConditionalLogBinomial, Projector=lb.Projector, SeedBinRegressor=lb.SeedBinRegressor,
              SeedBinRegressorUnnormed=lb.SeedBinRegressorUnnormed)
    ZoeDepth = ref_loader.extract_def("depth_modules/zoedepth/models/zoedepth/zoedepth_v1.py", "ZoeDepth", ns)
    conf = json.load(open(os.path.join(ref_loader.REF, "depth_modules/zoedepth/models/zoedepth/config_zoedepth.json")))["model"]

    class Core(nn.Module):
        output_channels = (256, 256, 256, 256, 256)

        def __init__(self):
            super().__init__()
            self.feats = None

        def forward(self, x, denorm=False, return_rel_depth=False):
            return self.feats[0], list(self.feats[1:])
    core = Core()
    model = ZoeDepth(core, **{k: v for k, v in conf.items() if k not in ("name", "version_name")}).eval()
    kinds = {}
    for mname, m in model.named_modules():
        if isinstance(m, nn.Conv2d):
            kinds[mname + '.weight'] = 'conv_w'; kinds[mname + '.bias'] = 'conv_b'
    sd = model.state_dict()
    for name, t in sd.items():
        if name in kinds:
            t.copy_(torch.from_numpy(synth_tensor('zoe.' + name, tuple(t.shape), kinds[name])))
    model.load_state_dict(sd)
    H, W = 64, 96
    g = np.random.default_rng(400)
    h16 = lambda a: a.astype(np.float16).astype(np.float32)          # fp16-representable values: the fixture stores them as float16
    rel = h16(g.uniform(0.2, 5.0, (1, H, W)))
    feats = [h16(g.normal(0, 1, (1, 32, H, W)))] + [h16(g.normal(0, 1, (1, 256, H >> s, W >> s))) for s in (5, 4, 3, 2, 1)]
    core.feats = [torch.from_numpy(rel)] + [torch.from_numpy(f) for f in feats]
    with torch.no_grad():
        out = model(torch.zeros(1, 3, H, W), return_final_centers=True)
    md, bc = out['metric_depth'].numpy(), out['bin_centers'].numpy()
    f16 = lambda a: a.astype(np.float16)
    np.savez_compressed(os.path.join(HERE, 'net_zoehead_64x96.npz'), rel=f16(rel), out_conv=f16(feats[0]), btlnck=f16(feats[1]),
                        r4=f16(feats[2]), r3=f16(feats[3]), r2=f16(feats[4]), r1=f16(feats[5]), metric_depth=md,
                        bin_centers=bc[:, ::8].copy())
    print('zoe head', md.shape, float(md.mean()), float(md.std()), float(bc.min()), float(bc.max()))


def zoe_infer_case():
    """The whole `depth_est: 'zoe'` call chain with the reference's OWN classes -- KenBurnsPipeline._depth_est_zoe
    (kenburns_effect.py:812-818, its text executed) -> DepthModel.infer (depth_model.py: reflect padding, flip TTA, bicubic resize
    back, crop) -> ZoeDepth.forward (zoedepth_v1.py) -> MidasCore.forward (midas.py: PrepForMidas resize + normalise, feature hooks)
    -- around a deterministic stand-in for the un-vendored MiDaS network (zoe_stub_core.py).  Stored: the image, what the core
    received in both TTA passes (= padding + flip + PrepForMidas), the metric depth and the disparity."""
    import itertools
    import json
    import types
    import zoe_stub_core as stub
    nn = torch.nn
    tvt = sys.modules['torchvision.transforms']

    class Normalize:                                # [EXT] torchvision.transforms.Normalize on a batched tensor: (x - mean) / std per channel
        def __init__(self, mean, std):
            self.mean, self.std = torch.tensor(mean).view(1, -1, 1, 1), torch.tensor(std).view(1, -1, 1, 1)

        def __call__(self, x):
            return (x - self.mean) / self.std
    tvt.Normalize = Normalize
    for n in ("depth_modules", "depth_modules.zoedepth", "depth_modules.zoedepth.models", "depth_modules.zoedepth.models.layers",
              "depth_modules.zoedepth.models.base_models"):
        ref_loader._bare(n)
    Lp = "depth_modules/zoedepth/models/"
    att = ref_loader.load_by_path("depth_modules.zoedepth.models.layers.attractor", Lp + "layers/attractor.py")
    dist = ref_loader.load_by_path("depth_modules.zoedepth.models.layers.dist_layers", Lp + "layers/dist_layers.py")
    lb = ref_loader.load_by_path("depth_modules.zoedepth.models.layers.localbins_layers", Lp + "layers/localbins_layers.py")
    dm = ref_loader.load_by_path("depth_modules.zoedepth.models.depth_model", Lp + "depth_model.py")
    mid = ref_loader.load_by_path("depth_modules.zoedepth.models.base_models.midas", Lp + "base_models/midas.py")
    ns = dict(torch=torch, nn=nn, itertools=itertools, DepthModel=dm.DepthModel, MidasCore=mid.MidasCore, load_state_from_resource=None,
              AttractorLayer=att.AttractorLayer, AttractorLayerUnnormed=att.AttractorLayerUnnormed,
              ConditionalLogBinomial=dist.ConditionalLogBinomial, Projector=lb.Projector, SeedBinRegressor=lb.SeedBinRegressor,
              SeedBinRegressorUnnormed=lb.SeedBinRegressorUnnormed)
    ZoeDepth = ref_loader.extract_def(Lp + "zoedepth/zoedepth_v1.py", "ZoeDepth", ns)
    conf = json.load(open(os.path.join(ref_loader.REF, Lp + "zoedepth/config_zoedepth.json")))["model"]

    class Fn(nn.Module):
        def __init__(self, f):
            super().__init__()
            self.f = f

        def forward(self, x):
            return self.f(x)

    class StubMidas(nn.Module):                     # the attribute layout MidasCore.attach_hooks walks (midas.py:302-325)
        def __init__(self):
            super().__init__()
            self.scratch = nn.Module()
            # output_conv's child [3] is the activation MidasCore calls "out_conv"; the last child stands for the final 1-channel conv
            # (it sees the prepared input through `self.x`: the stand-in's relative depth is a function of the input, like its features)
            self.scratch.output_conv = nn.Sequential(nn.Identity(), nn.Identity(), nn.Identity(), Fn(stub.out_conv),
                                                     Fn(lambda _act: stub.rel_depth(self.x)))
            self.scratch.layer4_rn = Fn(stub.layer4_rn)
            for lv in (4, 3, 2, 1):
                setattr(self.scratch, 'refinenet%d' % lv, Fn(lambda x, lv=lv: stub.refinenet(x, lv)))
            self.seen = []

        def forward(self, x):
            self.seen.append(x.clone())
            self.x = x
            self.scratch.layer4_rn(x)
            for lv in (4, 3, 2, 1):
                getattr(self.scratch, 'refinenet%d' % lv)(x)
            return self.scratch.output_conv(x)
    midas = StubMidas()
    NET = (96, 128)
    core = mid.MidasCore(midas, trainable=False, fetch_features=True, freeze_bn=True, keep_aspect_ratio=True, img_size=list(NET))
    core.output_channels = (256, 256, 256, 256, 256)
    model = ZoeDepth(core, **{k: v for k, v in conf.items() if k not in ("name", "version_name", "img_size")}).eval()
    kinds = {}
    for mname, m in model.named_modules():
        if isinstance(m, nn.Conv2d):
            kinds[mname + '.weight'] = 'conv_w'; kinds[mname + '.bias'] = 'conv_b'
    sd = model.state_dict()
    for name, t in sd.items():
        if name in kinds:
            t.copy_(torch.from_numpy(synth_tensor('zoe.' + name, tuple(t.shape), kinds[name])))
    model.load_state_dict(sd)
    g = np.random.default_rng(410)
    H, W = 70, 110
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = (0.5 + 0.35 * np.sin(xx[None] / 9.0 + np.arange(3).reshape(3, 1, 1)) * np.cos(yy[None] / 7.0)
           + g.uniform(-0.1, 0.1, (3, H, W))).clip(0, 1).astype(np.float32)[None]
    est = ref_loader.extract_def("anime_3dkenburns/kenburns_effect.py", "KenBurnsPipeline._depth_est_zoe", dict(torch=torch))
    fake_self = types.SimpleNamespace(depth_zoe=model, cfg=types.SimpleNamespace(focal=55.0, baseline=40.0), device='cpu')
    with torch.no_grad():
        depth = model.infer(torch.from_numpy(img), with_flip_aug=True, pad_input=True)
        n_seen = len(midas.seen)
        disparity = est(fake_self, torch.from_numpy(img))
    assert n_seen == 2
    np.savez_compressed(os.path.join(HERE, 'zoe_infer_70x110.npz'), img=img, net=np.array(NET), prep0=midas.seen[0].numpy(),
                        prep1=midas.seen[1].numpy(), depth=depth.numpy(), disparity=disparity.numpy(), focal=55.0, baseline=40.0)
    print('zoe infer', tuple(midas.seen[0].shape), tuple(depth.shape), float(depth.mean()), float(depth.std()), float(disparity.mean()))


if __name__ == '__main__':
    which = sys.argv[1:] or ['isnet', 'leres']
    if 'zoe' in which:
        zoe_head_case()
    if 'disparity' in which:
        disparity_case()
    if 'isnet' in which:
        isnet_cases()
    if 'leres' in which:
        leres_cases()
    if 'inpaint' in which:
        for h, w in INPAINT_SIZES:
            inpaint_case(h, w)
    if 'refine' in which:
        refine_case()
    if 'zoe_infer' in which:
        zoe_infer_case()

