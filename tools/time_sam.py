"""Times Segment Anything on one 1024x1024 image with synthetic weights: Sam.set_image and Sam.predict_boxes for 1, 10
and 100 boxes, for vit_b and vit_h; the time per kernel family from HIP events around every op of the two layer programs; the encoder's
fraction of the fp32 MFMA roof from the program's `flops`.  When `transformers` imports, the same SamModel configuration runs through
torch on the same GPU in fp32 as the comparison (random initialisation: only the time matters).

Medians of SAM_REPS passes (default 5) after a warm-up.  SAM_PRESETS=vit_b limits the presets.  Output -> profiles/sam_time.txt."""
import collections
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartoonsegmentation_amd import program as P, synth  # noqa: E402
from cartoonsegmentation_amd.nets.sam import PRESETS, SamConfig  # noqa: E402
from cartoonsegmentation_amd.sam import Sam  # noqa: E402
from cartoonsegmentation_amd.weights import SynthWeights  # noqa: E402

MFMA_FP32_ROOF = 157.3e12          # v_mfma_f32_32x32x2_f32 peak of one MI355X (include/csm355.h)
FAMILY = {P.OP_CONV: 'linear / conv (MFMA)', P.OP_LAYERNORM: 'layernorm', P.OP_ATTENTION_RELPOS: 'attention, decomposed bias',
          P.OP_CROSS_ATTENTION: 'cross-attention', P.OP_TOKENS: 'window / broadcast plumbing', P.OP_CHANNEL_DOT: 'hypernetwork product',
          P.OP_DEPTH_TO_SPACE: 'depth to space', P.OP_ADD: 'add / act', P.OP_ACT: 'add / act'}


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


def show(ms):
    return "median %.2f ms (min %.2f .. max %.2f, %d passes)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def families(cp, reps, out, *ext):
    per = [np.array(cp.profile(*ext)) for _ in range(reps)]
    med = np.median(np.stack(per), 0)
    fam = collections.OrderedDict()
    for o, ms in zip(cp.prog.ops, med):
        name = FAMILY.get(o['kind'], 'layout / other')
        if o['kind'] == P.OP_ATTENTION_RELPOS:
            name += ' (%d tokens)' % (o['kh'] * o['kw'])
        fam[name] = fam.get(name, 0.0) + float(ms)
    for name, ms in sorted(fam.items(), key=lambda kv: -kv[1]):
        out("      %-44s %8.3f ms" % (name, ms))
    return float(med.sum())


def hf_times(preset, img_t, box_sets, reps, out):
    try:
        from transformers import SamConfig as HFConfig, SamModel, SamVisionConfig
    except Exception as e:                                              # noqa: BLE001
        out("  transformers does not import here (%s): no torch comparison" % type(e).__name__)
        return
    p = PRESETS[preset]
    vc = SamVisionConfig(hidden_size=p['embed'], num_hidden_layers=p['depth'], num_attention_heads=p['heads'],
                         global_attn_indexes=list(p['global_blocks']))
    hc = HFConfig(vision_config=vc.to_dict())
    hc._attn_implementation = 'sdpa'
    m = SamModel(hc).float().cuda().eval()
    with torch.no_grad():
        emb = m.get_image_embeddings(img_t)
        out("  torch SamModel (fp32, sdpa) image encoder: %s" % show(timed(lambda: m.get_image_embeddings(img_t), reps)))
        for n, boxes in box_sets:
            b = boxes.reshape(1, n, 4)
            run = lambda: m(image_embeddings=emb, input_boxes=b, multimask_output=False)      # noqa: E731
            run()
            out("  torch SamModel prompt encoder + mask decoder, %3d boxes: %s" % (n, show(timed(run, reps))))
    del m
    torch.cuda.empty_cache()


def main():
    reps = max(5, int(os.environ.get("SAM_REPS", "5")))
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    img = torch.from_numpy(synth.image_u8(1024, 1024, 3)).cuda()
    g = np.random.default_rng(1)
    box_sets = []
    for n in (1, 10, 100):
        xy = g.uniform(0, 700, (n, 2))
        box_sets.append((n, torch.tensor(np.concatenate([xy, xy + g.uniform(60, 320, (n, 2))], 1), dtype=torch.float32, device='cuda')))
    out("Segment Anything, one 1024x1024 image, synthetic weights, fp32 (tools/time_sam.py; medians of %d passes after a warm-up)" % reps)
    for preset in os.environ.get("SAM_PRESETS", "vit_b,vit_h").split(","):
        cfg = SamConfig(preset)
        t0 = time.perf_counter()
        sam = Sam(SynthWeights('sam.'), 'cuda', cfg=cfg)
        sam.set_image(img)                                              # lowers and packs the encoder, tunes its conv tiles
        out("%s: encoder program %.1f GFLOP, %d ops; first set_image (lowering + packing + tile tuning) %.1f s"
            % (preset, sam.encoder().prog.flops / 1e9, len(sam.encoder().prog.ops), time.perf_counter() - t0))
        ms = timed(lambda: sam.set_image(img), reps)
        out("  set_image (preprocess + encoder): %s" % show(ms))
        out("    encoder per kernel family (HIP events around every op):")
        x = torch.empty((1, 3, 1024, 1024), device='cuda').normal_()
        enc_ms = families(sam.encoder(), reps, out, x, torch.empty((1, cfg.out_chans, cfg.grid, cfg.grid), device='cuda'))
        out("    encoder ops total %.2f ms = %.1f TFLOP/s = %.1f %% of the fp32 MFMA roof (%.1f TFLOP/s)"
            % (enc_ms, sam.encoder().prog.flops / enc_ms / 1e9, 100 * sam.encoder().prog.flops / (enc_ms * 1e-3) / MFMA_FP32_ROOF, MFMA_FP32_ROOF / 1e12))
        for n, boxes in box_sets:
            sam.predict_boxes(boxes)
            out("  predict_boxes, %3d boxes (chunks of %d): %s" % (n, sam.chunk_size(n), show(timed(lambda: sam.predict_boxes(boxes), reps))))
            if n == sam.chunk_size(n):
                out("    decoder per kernel family, batch %d:" % n)
                families(sam.decoder(n), reps, out, sam._emb, torch.empty((n, cfg.out_chans, cfg.n_tokens, 1), device='cuda').normal_(),
                         torch.empty((n, 1, 4 * cfg.grid, 4 * cfg.grid), device='cuda'), torch.empty((n, cfg.mask_tokens, 1, 1), device='cuda'))
        del sam
        torch.cuda.empty_cache()
        hf_times(preset, x, box_sets, reps, out)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sam_time.txt")
    dst = os.environ.get("SAM_TIME_OUT", path)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
