"""Segment Anything (Kirillov et al. 2023), box prompts only -> two layer programs: the ViT image encoder and the mask decoder.

The reference's `detector: sam` path calls `from sam import apply_sam`, a module it does not vendor, so this is a restatement of the
PUBLISHED definition [EXT]: segment_anything's modeling/{image_encoder.py, prompt_encoder.py, mask_decoder.py, transformer.py} with the
parameter names of its checkpoints (sam_vit_{b,l,h}_*.pth), as `SamPredictor.predict(box=..., multimask_output=False)` uses them.

  * image encoder: 16 x 16 patch convolution, learned absolute position embedding, pre-norm blocks (LayerNorm eps 1e-6, qkv with bias,
    attention with the decomposed relative position bias, proj, residual; LayerNorm, MLP with GELU, residual).  Blocks outside
    `global_blocks` zero-pad the g x g map to a multiple of the window AFTER the first LayerNorm, attend inside w x w windows (padded
    tokens are keys like any other: their k and v are the qkv bias) and drop the padding before the residual.  Neck: 1x1 convolution,
    LayerNorm over channels (eps 1e-6), 3x3 convolution, LayerNorm -- in NHWC a LayerNorm2d is the row LayerNorm.
  * prompt encoder: box corners + 0.5 -> [-1, 1] -> Gaussian matrix -> 2 pi -> sin | cos, + point_embeddings[2] / [3] (on the device:
    csm_sam_box_tokens); dense prompt = no_mask_embed; the grid's positional encoding is a constant of the model (computed at load, float64).
  * mask decoder: tokens [iou, 4 masks, 2 corners]; two-way transformer (2 layers, 8 heads, cross-attention at half width, ReLU MLP;
    LayerNorm eps 1e-5), final token -> image attention; ConvT 2x2 s2, LayerNorm2d, GELU, ConvT 2x2 s2, GELU; the hypernetwork MLP of mask
    token 0 times the upscaled map, and the IoU head.  multimask_output=False keeps mask 0 / IoU 0, so only that hypernetwork runs.
    One image embedding serves all boxes: the box is the decoder's batch dimension.

Lowering choices (tolerance-level, never silent): nn.Linear = 1x1 convolution on the fp32 MFMA engine; the attention scale d^-0.5 is folded
into the q rows of the projections (not a power of two at d = 80 or 32: one rounding of w * s instead of one of q * s); the relative
position tables are packed as R * sqrt(d) because the kernel multiplies them with the scaled q (CSM_OP_ATTENTION_RELPOS).  Tables whose
length is not 2 S - 1 for the block's window / grid size S are REFUSED: SAM never resamples at its fixed input size.
"""
import numpy as np

from ..program import Program

PRESETS = {
    'vit_b': dict(embed=768, depth=12, heads=12, global_blocks=(2, 5, 8, 11)),
    'vit_l': dict(embed=1024, depth=24, heads=16, global_blocks=(5, 11, 17, 23)),
    'vit_h': dict(embed=1280, depth=32, heads=16, global_blocks=(7, 15, 23, 31)),
}


class SamConfig:
    def __init__(self, preset=None, embed=768, depth=12, heads=12, global_blocks=(2, 5, 8, 11), window=14, patch=16, image=1024, out_chans=256,
                 mlp_dim=None, dec_heads=8, dec_depth=2, dec_mlp=2048, dec_downsample=2, iou_hidden=256, iou_depth=3, mask_tokens=4,
                 mask_in_chans=16, ln_eps=1e-6, dec_ln_eps=1e-5):
        if preset is not None:
            p = PRESETS[preset]
            embed, depth, heads, global_blocks = p['embed'], p['depth'], p['heads'], p['global_blocks']
        self.embed, self.depth, self.heads, self.global_blocks = embed, depth, heads, tuple(global_blocks)
        self.window, self.patch, self.image, self.out_chans = window, patch, image, out_chans
        self.mlp_dim = 4 * embed if mlp_dim is None else mlp_dim
        self.dec_heads, self.dec_depth, self.dec_mlp, self.dec_downsample = dec_heads, dec_depth, dec_mlp, dec_downsample
        self.iou_hidden, self.iou_depth, self.mask_tokens, self.mask_in_chans = iou_hidden, iou_depth, mask_tokens, mask_in_chans
        self.ln_eps, self.dec_ln_eps = ln_eps, dec_ln_eps
        assert embed % heads == 0 and image % patch == 0 and out_chans % 8 == 0 and out_chans % (dec_heads * dec_downsample) == 0

    grid = property(lambda s: s.image // s.patch)
    head_dim = property(lambda s: s.embed // s.heads)
    n_tokens = property(lambda s: 1 + s.mask_tokens + 2)


def _params(cfg):
    """every key of a segment_anything state dict for `cfg` -> (shape, synthetic-weight kind)"""
    E, g, C, d = cfg.embed, cfg.grid, cfg.out_chans, cfg.head_dim
    s = {'image_encoder.pos_embed': ((1, g, g, E), 'token'), 'image_encoder.patch_embed.proj.weight': ((E, 3, cfg.patch, cfg.patch), 'conv_w'),
         'image_encoder.patch_embed.proj.bias': ((E,), 'conv_b')}

    def lin(name, cout, cin):
        s[name + '.weight'], s[name + '.bias'] = ((cout, cin), 'lin_w'), ((cout,), 'conv_b')

    def norm(name, c):
        s[name + '.weight'], s[name + '.bias'] = ((c,), 'bn_gamma'), ((c,), 'bn_beta')

    def conv(name, cout, cin, k, bias=True):
        s[name + '.weight'] = ((cout, cin, k, k), 'conv_w')
        if bias:
            s[name + '.bias'] = ((cout,), 'conv_b')
    for i in range(cfg.depth):
        pre = 'image_encoder.blocks.%d.' % i
        S = g if i in cfg.global_blocks else cfg.window
        norm(pre + 'norm1', E); norm(pre + 'norm2', E)
        lin(pre + 'attn.qkv', 3 * E, E); lin(pre + 'attn.proj', E, E)
        s[pre + 'attn.rel_pos_h'] = s[pre + 'attn.rel_pos_w'] = ((2 * S - 1, d), 'lin_w')
        lin(pre + 'mlp.lin1', cfg.mlp_dim, E); lin(pre + 'mlp.lin2', E, cfg.mlp_dim)
    conv('image_encoder.neck.0', C, E, 1, bias=False); conv('image_encoder.neck.2', C, C, 3, bias=False)
    norm('image_encoder.neck.1', C); norm('image_encoder.neck.3', C)
    s['prompt_encoder.pe_layer.positional_encoding_gaussian_matrix'] = ((2, C // 2), 'unit')
    for k in range(4):
        s['prompt_encoder.point_embeddings.%d.weight' % k] = ((1, C), 'token')
    s['prompt_encoder.not_a_point_embed.weight'] = s['prompt_encoder.no_mask_embed.weight'] = ((1, C), 'token')
    m = cfg.mask_in_chans
    conv('prompt_encoder.mask_downscaling.0', m // 4, 1, 2); conv('prompt_encoder.mask_downscaling.3', m, m // 4, 2)
    conv('prompt_encoder.mask_downscaling.6', C, m, 1)
    norm('prompt_encoder.mask_downscaling.1', m // 4); norm('prompt_encoder.mask_downscaling.4', m)
    s['mask_decoder.iou_token.weight'], s['mask_decoder.mask_tokens.weight'] = ((1, C), 'token'), ((cfg.mask_tokens, C), 'token')

    def attn(name, inner):
        for pn in ('q_proj', 'k_proj', 'v_proj'):
            lin(name + '.' + pn, inner, C)
        lin(name + '.out_proj', C, inner)
    for i in range(cfg.dec_depth):
        pre = 'mask_decoder.transformer.layers.%d.' % i
        attn(pre + 'self_attn', C); attn(pre + 'cross_attn_token_to_image', C // cfg.dec_downsample)
        attn(pre + 'cross_attn_image_to_token', C // cfg.dec_downsample)
        for k in range(1, 5):
            norm(pre + 'norm%d' % k, C)
        lin(pre + 'mlp.lin1', cfg.dec_mlp, C); lin(pre + 'mlp.lin2', C, cfg.dec_mlp)
    attn('mask_decoder.transformer.final_attn_token_to_image', C // cfg.dec_downsample)
    norm('mask_decoder.transformer.norm_final_attn', C)
    conv('mask_decoder.output_upscaling.0', C, C // 4, 2, bias=False); conv('mask_decoder.output_upscaling.3', C // 4, C // 8, 2, bias=False)
    s['mask_decoder.output_upscaling.0.bias'] = ((C // 4,), 'conv_b')                    # (ConvTranspose2d: weight [cin, cout, k, k])
    s['mask_decoder.output_upscaling.3.bias'] = ((C // 8,), 'conv_b')
    norm('mask_decoder.output_upscaling.1', C // 4)
    for i in range(cfg.mask_tokens):
        pre = 'mask_decoder.output_hypernetworks_mlps.%d.layers.' % i
        lin(pre + '0', C, C); lin(pre + '1', C, C); lin(pre + '2', C // 8, C)
    dims = [C] + [cfg.iou_hidden] * (cfg.iou_depth - 1) + [cfg.mask_tokens]
    for k in range(cfg.iou_depth):
        lin('mask_decoder.iou_prediction_head.layers.%d' % k, dims[k + 1], dims[k])
    return s


def sam_param_shapes(cfg):
    """every key of a segment_anything state dict for `cfg` -> shape (the prompt encoder's mask branch and not_a_point_embed included:
    checkpoints carry them, the box-only path does not read them)"""
    return {k: v[0] for k, v in _params(cfg).items()}


UNUSED_KEYS = ('prompt_encoder.mask_downscaling.', 'prompt_encoder.not_a_point_embed.', 'prompt_encoder.point_embeddings.0.',
               'prompt_encoder.point_embeddings.1.')        # point / mask prompts; hypernetworks 1.. and IoU 1.. belong to multimask_output=True


def synth_state_dict(ws, cfg):
    """a complete segment_anything-named state dict drawn from a weight source (SynthWeights): what a checkpoint file would hold"""
    return {k: ws.get(k, shp, kind) for k, (shp, kind) in _params(cfg).items()}


def infer_config(sd, **overrides):
    """SamConfig from the shapes of a segment_anything state dict: width, depth, heads (from rel_pos's head dimension), global blocks (the
    blocks whose tables are longer than the others'), window, patch, image size; vit_b / vit_l / vit_h come out as their presets"""
    shp = lambda k: tuple(int(v) for v in sd[k].shape)           # noqa: E731
    E, _, patch, _ = shp('image_encoder.patch_embed.proj.weight')
    g = shp('image_encoder.pos_embed')[1]
    depth = 1 + max(int(k.split('.')[2]) for k in sd if k.startswith('image_encoder.blocks.'))
    lens = [shp('image_encoder.blocks.%d.attn.rel_pos_h' % i)[0] for i in range(depth)]
    d = shp('image_encoder.blocks.0.attn.rel_pos_h')[1]
    glob = tuple(i for i, n in enumerate(lens) if n == 2 * g - 1 and n != min(lens)) if min(lens) != max(lens) else tuple(range(depth))
    window = (min(lens) + 1) // 2 if min(lens) != max(lens) else 0
    C = shp('image_encoder.neck.0.weight')[0]
    kw = dict(embed=E, depth=depth, heads=E // d, global_blocks=glob, window=window or g, patch=patch, image=g * patch, out_chans=C,
              mlp_dim=shp('image_encoder.blocks.0.mlp.lin1.weight')[0], dec_mlp=shp('mask_decoder.transformer.layers.0.mlp.lin1.weight')[0],
              dec_depth=1 + max(int(k.split('.')[3]) for k in sd if k.startswith('mask_decoder.transformer.layers.')),
              dec_downsample=C // shp('mask_decoder.transformer.layers.0.cross_attn_token_to_image.q_proj.weight')[0],
              iou_hidden=shp('mask_decoder.iou_prediction_head.layers.0.weight')[0],
              iou_depth=1 + max(int(k.split('.')[3]) for k in sd if k.startswith('mask_decoder.iou_prediction_head.layers.')),
              mask_tokens=shp('mask_decoder.mask_tokens.weight')[0])
    kw.update(overrides)
    return SamConfig(**kw)


def preset_of(cfg):
    for name, p in PRESETS.items():
        if (cfg.embed, cfg.depth, cfg.heads, tuple(cfg.global_blocks)) == (p['embed'], p['depth'], p['heads'], p['global_blocks']):
            return name
    return None


def _rel_table(ws, name, S, d):
    """a relative position table as the block needs it: [2 S - 1, d], anything else refused"""
    try:
        return ws.get(name, (2 * S - 1, d), 'lin_w')
    except AssertionError as e:
        raise ValueError("%s: a relative position table of %d rows x %d is required for a window / grid of %d (SAM does not resample its "
                         "tables at its fixed input size): %s" % (name, 2 * S - 1, d, S, e))


def _lin(ws, name, cout, cin):
    return ws.get(name + '.weight', (cout, cin), 'lin_w'), ws.get(name + '.bias', (cout,), 'conv_b')


def _norm(p, ws, x, name, eps):
    return p.layernorm(x, ws.get(name + '.weight', (x.c,), 'bn_gamma'), ws.get(name + '.bias', (x.c,), 'bn_beta'), eps)


def build_sam_encoder(ws, cfg, n=1):
    """ext tensors (NCHW): [0] the normalised, zero-padded input [n, 3, S, S]; [1] the image embedding [n, out_chans, g, g]"""
    E, heads, d, g, w = cfg.embed, cfg.heads, cfg.head_dim, cfg.grid, cfg.window
    p = Program("sam_encoder")
    x_ext = p.ext_nchw(n, 3, cfg.image, cfg.image)
    out_ext = p.ext_nchw(n, cfg.out_chans, g, g)
    pre = 'image_encoder.'
    x = p.to_nhwc(x_ext)
    t = p.conv(x, ws.get(pre + 'patch_embed.proj.weight', (E, 3, cfg.patch, cfg.patch), 'conv_w'),
               ws.get(pre + 'patch_embed.proj.bias', (E,), 'conv_b'), stride=cfg.patch)
    t = p.broadcast_add(t, const=ws.get(pre + 'pos_embed', (1, g, g, E), 'token'), per_position=True)
    scale = np.float32(d) ** np.float32(-0.5)
    for i in range(cfg.depth):
        b = pre + 'blocks.%d.' % i
        glob = i in cfg.global_blocks
        S = g if glob else w
        y = _norm(p, ws, t, b + 'norm1', cfg.ln_eps)
        qw, qb = _lin(ws, b + 'attn.qkv', 3 * E, E)
        qw, qb = qw.copy(), qb.copy()
        qw[:E] *= scale; qb[:E] *= scale
        rh, rw = _rel_table(ws, b + 'attn.rel_pos_h', S, d), _rel_table(ws, b + 'attn.rel_pos_w', S, d)
        ow, ob = _lin(ws, b + 'attn.proj', E, E)
        if glob:
            t = p.linear(p.attention_relpos(p.linear(y, qw, qb), heads, (g, g), rh, rw), ow, ob, res=t)
        else:
            a = p.attention_relpos(p.linear(p.window_partition(y, w), qw, qb), heads, (w, w), rh, rw)
            t = p.window_unpartition(p.linear(a, ow, ob), w, t, res=t)
        y = _norm(p, ws, t, b + 'norm2', cfg.ln_eps)
        w1, b1 = _lin(ws, b + 'mlp.lin1', cfg.mlp_dim, E)
        w2, b2 = _lin(ws, b + 'mlp.lin2', E, cfg.mlp_dim)
        t = p.linear(p.linear(y, w1, b1, act='gelu'), w2, b2, res=t)
    C = cfg.out_chans
    y = _norm(p, ws, p.conv(t, ws.get(pre + 'neck.0.weight', (C, E, 1, 1), 'conv_w'), None), pre + 'neck.1', 1e-6)
    y = _norm(p, ws, p.conv(y, ws.get(pre + 'neck.2.weight', (C, C, 3, 3), 'conv_w'), None, pad=1), pre + 'neck.3', 1e-6)
    p.to_nchw(y, out_ext)
    p.plan()
    return p


def dense_pe(gauss, g):
    """PositionEmbeddingRandom.forward((g, g)): [g, g, C] float32, computed in float64"""
    gauss = np.asarray(gauss, np.float64)
    c = (np.arange(g, dtype=np.float64) + 0.5) / g
    xy = np.stack(np.broadcast_arrays(c[None, :], c[:, None]), -1)            # [g, g, (x, y)]
    arg = 2.0 * np.pi * ((2.0 * xy - 1.0) @ gauss)
    return np.concatenate([np.sin(arg), np.cos(arg)], -1).astype(np.float32)


def prompt_constants(ws, cfg):
    """the device constants of csm_sam_box_tokens: [1 + mask_tokens][C] output tokens, [2][C] corner embeddings, [2][C / 2] Gaussian matrix"""
    C = cfg.out_chans
    return np.concatenate([ws.get('mask_decoder.iou_token.weight', (1, C), 'token').reshape(-1),
                           ws.get('mask_decoder.mask_tokens.weight', (cfg.mask_tokens, C), 'token').reshape(-1),
                           ws.get('prompt_encoder.point_embeddings.2.weight', (1, C), 'token').reshape(-1),
                           ws.get('prompt_encoder.point_embeddings.3.weight', (1, C), 'token').reshape(-1),
                           ws.get('prompt_encoder.pe_layer.positional_encoding_gaussian_matrix', (2, C // 2), 'unit').reshape(-1)]).astype(np.float32)


def build_sam_decoder(ws, cfg, n):
    """ext tensors (NCHW): [0] image embedding [1, C, g, g]; [1] decoder tokens [n, C, T, 1] (csm_sam_box_tokens); outputs [2] low-res logits
    of mask 0 [n, 1, 4g, 4g]; [3] IoU predictions [n, mask_tokens, 1, 1] (multimask_output=False reads channel 0)"""
    C, g, T, heads = cfg.out_chans, cfg.grid, cfg.n_tokens, cfg.dec_heads
    p = Program("sam_decoder")
    emb_ext = p.ext_nchw(1, C, g, g)
    tok_ext = p.ext_nchw(n, C, T, 1)
    lg_ext = p.ext_nchw(n, 1, 4 * g, 4 * g)
    iou_ext = p.ext_nchw(n, cfg.mask_tokens, 1, 1)
    tok = p.to_nhwc(tok_ext)                                                    # [n, T, 1, C]: the queries' positional part throughout
    keys = p.broadcast_add(p.to_nhwc(emb_ext), const=ws.get('prompt_encoder.no_mask_embed.weight', (1, C), 'token'), n=n)
    pe = dense_pe(ws.get('prompt_encoder.pe_layer.positional_encoding_gaussian_matrix', (2, C // 2), 'unit'), g)

    def attn(name, q_in, k_in, v_in, inner, res=None):
        d = inner // heads
        s = np.float32(d) ** np.float32(-0.5)
        qw, qb = _lin(ws, name + '.q_proj', inner, C)
        kw, kb = _lin(ws, name + '.k_proj', inner, C)
        vw, vb = _lin(ws, name + '.v_proj', inner, C)
        ow, ob = _lin(ws, name + '.out_proj', C, inner)
        kv = p.buffer(k_in.n, k_in.h, k_in.w, 2 * inner)
        p.linear(k_in, kw, kb, out=kv.slice(0, inner))
        p.linear(v_in, vw, vb, out=kv.slice(inner, 2 * inner))
        return p.linear(p.cross_attention(p.linear(q_in, qw * s, qb * s), kv, heads), ow, ob, res=res)

    q = tok
    for i in range(cfg.dec_depth):
        b = 'mask_decoder.transformer.layers.%d.' % i
        if i == 0:                                                              # skip_first_layer_pe: no positional add, no residual
            q = attn(b + 'self_attn', q, q, q, C)
        else:
            qq = p.add(q, tok)
            q = attn(b + 'self_attn', qq, qq, q, C, res=q)
        q = _norm(p, ws, q, b + 'norm1', cfg.dec_ln_eps)
        kk = p.broadcast_add(keys, const=pe, per_position=True)
        q = _norm(p, ws, attn(b + 'cross_attn_token_to_image', p.add(q, tok), kk, keys, C // cfg.dec_downsample, res=q), b + 'norm2', cfg.dec_ln_eps)
        w1, b1 = _lin(ws, b + 'mlp.lin1', cfg.dec_mlp, C)
        w2, b2 = _lin(ws, b + 'mlp.lin2', C, cfg.dec_mlp)
        q = _norm(p, ws, p.linear(p.linear(q, w1, b1, act='relu'), w2, b2, res=q), b + 'norm3', cfg.dec_ln_eps)
        keys = _norm(p, ws, attn(b + 'cross_attn_image_to_token', kk, p.add(q, tok), q, C // cfg.dec_downsample, res=keys), b + 'norm4',
                     cfg.dec_ln_eps)
    kk = p.broadcast_add(keys, const=pe, per_position=True)
    q = _norm(p, ws, attn('mask_decoder.transformer.final_attn_token_to_image', p.add(q, tok), kk, keys, C // cfg.dec_downsample, res=q),
              'mask_decoder.transformer.norm_final_attn', cfg.dec_ln_eps)

    # ---- upscaling, hypernetwork of mask token 0, IoU head
    u = 'mask_decoder.output_upscaling.'
    up = p.conv_transpose_nonoverlap(keys, ws.get(u + '0.weight', (C, C // 4, 2, 2), 'conv_w'), ws.get(u + '0.bias', (C // 4,), 'conv_b'), 2)
    up = p.act(_norm(p, ws, up, u + '1', 1e-6), 'gelu')
    w3 = ws.get(u + '3.weight', (C // 4, C // 8, 2, 2), 'conv_w')
    up = p.depth_to_space(p.conv(up, w3.transpose(2, 3, 1, 0).reshape(4 * (C // 8), C // 4, 1, 1),
                                 np.tile(ws.get(u + '3.bias', (C // 8,), 'conv_b'), 4), act='gelu'), 2)     # (GELU commutes with the scatter)
    flat = p.reshape(q, n, 1, 1, T * C)

    def mlp(name, x, dims):
        for k in range(len(dims) - 1):
            wk, bk = _lin(ws, name + '.layers.%d' % k, dims[k + 1], dims[k])
            x = p.linear(x, wk, bk, act='relu' if k < len(dims) - 2 else None)
        return x
    hyper = mlp('mask_decoder.output_hypernetworks_mlps.0', flat.slice(C, 2 * C), [C, C, C, C // 8])
    p.to_nchw(p.channel_dot(up, hyper), lg_ext)
    p.to_nchw(mlp('mask_decoder.iou_prediction_head', flat.slice(0, C), [C] + [cfg.iou_hidden] * (cfg.iou_depth - 1) + [cfg.mask_tokens]), iou_ext)
    p.plan()
    return p
