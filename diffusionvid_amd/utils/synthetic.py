"""Seeded synthetic weights, frames and noise (there is no checkpoint or dataset in the build box).

Shapes and names follow the reference state_dict contract: `backbone.bottom_up.*`,
`backbone.fpn_*` (detectron2 names) and `head.*` (mega_core/modeling/roi_heads/box_head/box_head.py).
Head init mirrors DynamicHead._reset_parameters (box_head.py:239-248): xavier_uniform_ for every
matrix, focal-prior bias on class_logits; norms/biases get small random values so that a kernel
which ignores an affine term cannot pass parity.  Backbone: He-normal convs with FrozenBN
statistics chosen so activations stay O(1) through 33 residual blocks (fp16-safe).
"""
import math

import torch


def _xavier(g, out_f, in_f):
    bound = math.sqrt(6.0 / (in_f + out_f))
    return (torch.rand(out_f, in_f, generator=g) * 2 - 1) * bound


def _bias(g, n, fan_in):
    b = 1.0 / math.sqrt(fan_in)
    return (torch.rand(n, generator=g) * 2 - 1) * b


def _ln(g, sd, name, d):
    sd[name + ".weight"] = torch.rand(d, generator=g) * 0.6 + 0.7
    sd[name + ".bias"] = (torch.rand(d, generator=g) * 2 - 1) * 0.2


def make_head_state_dict(seed=0, hidden=256, nheads=8, dim_ff=2048, dim_dynamic=64, num_classes=30, num_cls=1, num_reg=3,
                         num_heads=3, num_heads_cond=1, pooler=7, prior_prob=0.01, prefix="head.", local_stages=0):
    """local_stages > 0 adds `local_attention.{i}.0.*` (MultiheadAttention) and `local_attention.{i}.2.*` (LayerNorm) for i < local_stages
    (box_head.py:186-194; entry 1 of each stage is a Dropout, which has no parameters).  They are drawn AFTER every other tensor, so the
    rest of the dict is bit-identical whatever local_stages is."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    d = hidden

    def linear(name, out_f, in_f, bias=True):
        sd[name + ".weight"] = _xavier(g, out_f, in_f)
        if bias:
            sd[name + ".bias"] = _bias(g, out_f, in_f)

    def mha(name):
        sd[name + ".in_proj_weight"] = _xavier(g, 3 * d, d)
        sd[name + ".in_proj_bias"] = (torch.rand(3 * d, generator=g) * 2 - 1) * 0.1
        sd[name + ".out_proj.weight"] = _xavier(g, d, d)
        sd[name + ".out_proj.bias"] = (torch.rand(d, generator=g) * 2 - 1) * 0.1

    def head(p, cond):
        mha(p + ".self_attn")
        linear(p + ".inst_interact.dynamic_layer", 2 * d * dim_dynamic, d)
        _ln(g, sd, p + ".inst_interact.norm1", dim_dynamic)
        _ln(g, sd, p + ".inst_interact.norm2", d)
        linear(p + ".inst_interact.out_layer", d, d * pooler * pooler)
        _ln(g, sd, p + ".inst_interact.norm3", d)
        linear(p + ".linear1", dim_ff, d)
        linear(p + ".linear2", d, dim_ff)
        for n in ("norm1", "norm2", "norm3"):
            _ln(g, sd, f"{p}.{n}", d)
        linear(p + ".block_time_mlp.1", d if cond else 2 * d, 4 * d)
        for i in range(num_cls):
            linear(f"{p}.cls_module.{3 * i}", d, d, bias=False)
            _ln(g, sd, f"{p}.cls_module.{3 * i + 1}", d)
        for i in range(num_reg):
            linear(f"{p}.reg_module.{3 * i}", d, d, bias=False)
            _ln(g, sd, f"{p}.reg_module.{3 * i + 1}", d)
        linear(p + ".class_logits", num_classes, d)
        sd[p + ".class_logits.bias"] = torch.full((num_classes,), -math.log((1 - prior_prob) / prior_prob))
        linear(p + ".bboxes_delta", 4, d)
        if cond:
            linear(p + ".c_mlp.1", d, d)

    for i in range(num_heads):
        head(f"{prefix}head_series.{i}", False)
    for i in range(num_heads_cond):
        head(f"{prefix}head_series_cond.{i}", True)
    mha(prefix + "global_attention.0.0")
    linear(prefix + "time_mlp.1", 4 * d, d)
    linear(prefix + "time_mlp.3", 4 * d, 4 * d)
    for i in range(local_stages):
        mha(f"{prefix}local_attention.{i}.0")
        _ln(g, sd, f"{prefix}local_attention.{i}.2", d)
    return sd


def _check_fpn_levels(fpn_levels):
    if tuple(fpn_levels) not in ((3, 4, 5), (2, 3, 4, 5)):
        raise ValueError("fpn_levels must be (3, 4, 5) or (2, 3, 4, 5), got %r" % (tuple(fpn_levels),))
    return tuple(fpn_levels)


def _fpn_level(g, sd, prefix, lvl, c, out_channels):
    sd[f"{prefix}fpn_lateral{lvl}.weight"] = (torch.rand(out_channels, c, 1, 1, generator=g) * 2 - 1) * math.sqrt(3.0 / c)
    sd[f"{prefix}fpn_lateral{lvl}.bias"] = (torch.rand(out_channels, generator=g) * 2 - 1) * 0.05
    fan = out_channels * 9
    sd[f"{prefix}fpn_output{lvl}.weight"] = (torch.rand(out_channels, out_channels, 3, 3, generator=g) * 2 - 1) * math.sqrt(3.0 / fan)
    sd[f"{prefix}fpn_output{lvl}.bias"] = (torch.rand(out_channels, generator=g) * 2 - 1) * 0.05


def make_backbone_state_dict(seed=1, blocks=(3, 4, 23, 3), out_channels=256, prefix="backbone.", fpn_levels=(3, 4, 5)):
    """fpn_levels (2, 3, 4, 5) adds the stride-4 level's fpn_lateral2 / fpn_output2, drawn after everything else: a seed's other values
    do not depend on it."""
    fpn_levels = _check_fpn_levels(fpn_levels)
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv_bn(name, cout, cin, k, gamma=(0.8, 1.2)):
        fan_in = cin * k * k
        sd[name + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / fan_in)
        sd[name + ".norm.weight"] = torch.rand(cout, generator=g) * (gamma[1] - gamma[0]) + gamma[0]
        sd[name + ".norm.bias"] = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
        sd[name + ".norm.running_mean"] = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
        sd[name + ".norm.running_var"] = torch.rand(cout, generator=g) * 0.4 + 0.8

    bu = prefix + "bottom_up."
    conv_bn(bu + "stem.conv1", 64, 3, 7)
    cin = 64
    for s, nb in enumerate(blocks):
        width, cout = 64 << s, 256 << s
        for b in range(nb):
            p = f"{bu}res{s + 2}.{b}"
            conv_bn(p + ".conv1", width, cin, 1)
            conv_bn(p + ".conv2", width, width, 3)
            conv_bn(p + ".conv3", cout, width, 1, gamma=(0.2, 0.4))   # damp the residual branch
            if b == 0:
                conv_bn(p + ".shortcut", cout, cin, 1)
            cin = cout
    for lvl, c in zip((3, 4, 5), (512, 1024, 2048)):
        _fpn_level(g, sd, prefix, lvl, c, out_channels)
    if 2 in fpn_levels:
        _fpn_level(g, sd, prefix, 2, 256, out_channels)
    return sd


def make_swin_state_dict(seed=1, embed_dim=128, depths=(2, 2, 18, 2), heads=(4, 8, 16, 32), window=7, out_channels=256,
                         prefix="backbone.", fpn_levels=(3, 4, 5)):
    """Swin-Transformer + FPN parameters under the reference's names (swintransformer.py modules wrapped by
    detectron2's FPN as `backbone.bottom_up.*`).  Values are O(1)-preserving random (not the std-0.02 default).  fpn_levels
    (2, 3, 4, 5) adds stage 0's output norm (norm0, out_indices (0, 1, 2, 3)) and fpn_lateral2 / fpn_output2, drawn after everything else."""
    fpn_levels = _check_fpn_levels(fpn_levels)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    bu = prefix + "bottom_up."

    def lin(name, o, i, bias=True):
        sd[name + ".weight"] = torch.randn(o, i, generator=g) / math.sqrt(i)
        if bias:
            sd[name + ".bias"] = (torch.rand(o, generator=g) * 2 - 1) * 0.2

    sd[bu + "patch_embed.proj.weight"] = torch.randn(embed_dim, 3, 4, 4, generator=g) / math.sqrt(48)
    sd[bu + "patch_embed.proj.bias"] = (torch.rand(embed_dim, generator=g) * 2 - 1) * 0.2
    _ln(g, sd, bu + "patch_embed.norm", embed_dim)
    for i, depth in enumerate(depths):
        C = embed_dim << i
        for j in range(depth):
            p = f"{bu}layers.{i}.blocks.{j}"
            _ln(g, sd, p + ".norm1", C)
            _ln(g, sd, p + ".norm2", C)
            lin(p + ".attn.qkv", 3 * C, C)
            lin(p + ".attn.proj", C, C)
            sd[p + ".attn.proj.weight"] *= 0.5            # keep the residual stream from exploding over 24 blocks
            sd[p + ".attn.relative_position_bias_table"] = torch.randn((2 * window - 1) ** 2, heads[i], generator=g) * 0.5
            lin(p + ".mlp.fc1", 4 * C, C)
            lin(p + ".mlp.fc2", C, 4 * C)
            sd[p + ".mlp.fc2.weight"] *= 0.5
        if i < len(depths) - 1:
            _ln(g, sd, f"{bu}layers.{i}.downsample.norm", 4 * C)
            lin(f"{bu}layers.{i}.downsample.reduction", 2 * C, 4 * C, bias=False)
        if i >= 1:
            _ln(g, sd, f"{bu}norm{i}", C)
    for lvl, i in zip((3, 4, 5), (1, 2, 3)):
        _fpn_level(g, sd, prefix, lvl, embed_dim << i, out_channels)
    if 2 in fpn_levels:
        _ln(g, sd, f"{bu}norm0", embed_dim)
        _fpn_level(g, sd, prefix, 2, embed_dim, out_channels)
    return sd


def make_state_dict(seed=0, blocks=(3, 4, 23, 3), swin=None, fpn_levels=(3, 4, 5), **head_kw):
    sd = make_head_state_dict(seed, **head_kw)
    if swin is not None:
        sd.update(make_swin_state_dict(seed + 1, **swin, fpn_levels=fpn_levels))
    else:
        sd.update(make_backbone_state_dict(seed + 1, blocks, fpn_levels=fpn_levels))
    return sd


def synthetic_frame(index, height=600, width=1000, video=0, smooth=False):
    """torch.rand(3,600,1000) fp32 in [0,1), seed 1000+i (post-ToTensor domain).

    smooth=True gives a low-frequency image instead (bicubic upsampling of a coarse random grid):
    with white-noise frames and random weights the 3-stage box refinement is chaotic (an fp16 rounding
    of the feature maps alone moves stage-3 outputs by O(1), measured on the CPU oracle), which makes
    end-to-end parity meaningless; the end-to-end parity tests therefore use smooth frames."""
    g = torch.Generator().manual_seed(1000 + index + 100003 * video)
    if not smooth:
        return torch.rand(3, height, width, generator=g)
    coarse = torch.rand(1, 3, max(2, height // 32), max(2, width // 32), generator=g)
    img = torch.nn.functional.interpolate(coarse, size=(height, width), mode="bicubic", align_corners=False)
    return img[0].clamp_(0, 1)


def tame_box_deltas(state_dict, gain=0.1):
    """Scale every `bboxes_delta` layer (weight and bias) by `gain` -- random-init heads otherwise
    multiply box sizes by e^(+-2) per stage, unlike a trained model whose refinements shrink."""
    out = dict(state_dict)
    for k, v in state_dict.items():
        if ".bboxes_delta." in k:
            out[k] = v * gain
    return out


def trained_like_scores(state_dict, gain=2.5, bias=-6.5):
    """Class layers shaped like a trained detector's instead of the focal-prior initialisation: every `class_logits.weight`
    times `gain`, every `class_logits.bias` set to `bias`.  At initialisation the logits are -4.5 +- 0.95 (measured on the CPU
    oracle): sigmoid scores with median 0.01, the 300th of a frame's 9000 candidates near 0.07 and none above 0.26 -- nothing
    ever crosses the 0.5 renewal threshold of the DDIM loop (diffusion_det.py:559-572) and the whole top-300 sits in a band
    a few score tolerances wide.  With gain 2.5 and bias -6.5 the final-stage logits are -6.7 +- 2.4: scores from 1e-4 to
    ~0.8, the 300th near 0.16, the best box of a frame at 0.55-0.8, and 2-11 boxes per frame above 0.5 -- the x4 sampler keeps
    some boxes and refills the rest, and NMS orders real score gaps.  The gain also multiplies every fp16-vs-fp32 logit
    difference by 2.5, i.e. the tolerance is tested where it binds."""
    out = dict(state_dict)
    for k, v in state_dict.items():
        if k.endswith(".class_logits.weight"):
            out[k] = v * gain
        elif k.endswith(".class_logits.bias"):
            out[k] = torch.full_like(v, bias)
    return out


# The training draws (DiffusionDet.compute_losses) are kinds 4 .. 7.  The key has two bits for the kind, so they reuse the four slots on a video
# number 50021 higher: every key of the kinds 0 .. 3 is what it was, and a training draw meets an inference draw only across videos 50021 apart.
_KINDS = {"box_init": 0, "img": 1, "ddim": 2, "renew": 3, "train_t": 4, "train_noise": 5, "train_placeholder": 6, "train_uncond": 7}


def draw_key(kind, frame_id, step, image, video=0):
    k = _KINDS[kind]
    return 2000 + (((((video + 50021 * (k >> 2)) * 100003 + frame_id) * 4 + (k & 3)) * 64 + step) * 64 + image)


def noise_fn(kind, frame_id, step, image, shape, video=0):
    """Injected N(0,1) draws shared by the CPU oracle and the GPU path (the reference draws them on
    the device at diffusion_det.py:449,:542,:587,:595).  Keyed by (video, call frame, kind, step,
    image), not by RNG stream position, so 8-frame batches can be sharded across ranks."""
    seed = draw_key(kind, frame_id, step, image, video)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


class DeviceNoise:
    """`model.noise_fn = DeviceNoise()`: the detector draws on the DEVICE (ops.counter_normal -> dvid_counter_normal: Philox4x32-10
    keyed like `noise_fn` above, fp64 Box-Muller) instead of calling a host generator and uploading -- no host RNG time, no
    pageable H2D copies (41 per video with the host draws), and still a pure function of (video, call frame, kind, step, image):
    ranks that share a video draw the same values, and the CPU oracle regenerates them (oracle/noise.py).  Calling the object
    returns the same draw as a device tensor, so code that expects a `noise_fn` keeps working."""
    on_device = True

    def __init__(self, video=0):
        self.video = video

    def key(self, kind, frame_id, step, image):
        return draw_key(kind, frame_id, step, image, self.video)

    def draw(self, kind, frame_id, step, first_image, n_images, shape, device=None):
        from .. import ops
        return ops.counter_normal(self.key(kind, frame_id, step, first_image), n_images, shape, device)

    def draw_ids(self, kind, ids, step, shape, device=None, image=0):
        """[len(ids), *shape]: the draws keyed (kind, id, step, `image`) of a batch of still images (`image`: the view index under
        TEST.BBOX_AUG, 0 for the plain image) -- ONE launch when the ids are
        consecutive (their keys lie a fixed stride apart), else one per run of consecutive ids"""
        import torch
        from .. import ops
        ids = [int(i) for i in ids]
        stride = self.key(kind, 1, step, 0) - self.key(kind, 0, step, 0)
        runs, a = [], 0
        for b in range(1, len(ids) + 1):
            if b == len(ids) or ids[b] != ids[b - 1] + 1:
                runs.append(ops.counter_normal(self.key(kind, ids[a], step, image), b - a, shape, device, key_stride=stride))
                a = b
        return runs[0] if len(runs) == 1 else torch.cat(runs)

    def __call__(self, kind, frame_id, step, image, shape, video=None):
        return self.draw(kind, frame_id, step, image, 1, shape)[0]
