"""Shared inputs of the four-level (p2..p5) pyramid tests: the box recipe that reaches every level, and the level-2 tensor names."""
import torch

STRIDES4 = (4, 8, 16, 32)
SCALES4 = (1 / 4., 1 / 8., 1 / 16., 1 / 32.)
LEVEL2_RESNET = ("backbone.fpn_lateral2.weight", "backbone.fpn_lateral2.bias", "backbone.fpn_output2.weight", "backbone.fpn_output2.bias")
LEVEL2_SWIN = LEVEL2_RESNET + ("backbone.bottom_up.norm0.weight", "backbone.bottom_up.norm0.bias")
RES4 = ("res2", "res3", "res4", "res5")
MEAN, STD = (123.675, 116.280, 103.530), (58.395, 57.120, 57.375)


def maps_and_boxes(seed=4, n=2, M=96, H=160, W=256, c=256):
    """fp32 NCHW maps at strides 4, 8, 16, 32 (drawn in that order), and boxes [n, M, 4]: centres rand * [W, H] * 1.2 - [W, H] * 0.1, sizes
    exp(rand * 3.6 + 3.0), i.e. sides from 20 to 735 pixels -- both sides of every level threshold (112, 224, 448).  The maps and the
    boxes each come from their own generator with this seed: the level counts the tests assert (75 / 64 / 43 / 10 at the defaults) are
    those of the boxes drawn first from a fresh generator; drawn behind the maps from one generator the same formulas leave level 5 with
    4 boxes, short of the 10 the tests require.  -> (a generator for further draws, maps, boxes)."""
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(n, c, H // s, W // s, generator=g) for s in STRIDES4]
    gb = torch.Generator().manual_seed(seed)
    cxcy = torch.rand(n, M, 2, generator=gb) * torch.tensor([W, H]) * 1.2 - torch.tensor([W, H]) * 0.1
    wh = torch.exp(torch.rand(n, M, 2, generator=gb) * 3.6 + 3.0)
    boxes = torch.cat([cxcy - wh / 2, cxcy + wh / 2], dim=-1)
    return g, feats, boxes


def with_edge_boxes(boxes, H, W):
    b = boxes.clone()
    b[0, 0] = torch.tensor([10.0, 10.0, 10.0, 10.0])          # zero area
    b[0, 1] = torch.tensor([-50.0, -40.0, W + 80.0, H + 60.0])  # larger than the image
    b[0, 2] = torch.tensor([W - 3.0, H - 3.0, W + 40.0, H + 40.0])
    return b


def level_counts(boxes):
    from oracle import roi_align as oroi
    return torch.bincount(oroi.assign_boxes_to_levels(boxes.reshape(-1, 4), 2, 5), minlength=4).tolist()


# ---- closed-form RoIAlignV2 answers on affine maps, four levels (in the manner of tests/test_known_answers.py) -----------------------
KA_IMG = 512
KA_BOXES = [          # (what it pins, box xyxy, expected level)
    ("111 x 112, sqrt(area) below 112: level 2", [100.0, 100.0, 211.0, 212.0], 2),
    ("sqrt(area) = 112 exactly: first size of level 3", [200.0, 200.0, 312.0, 312.0], 3),
    ("sqrt(area) = 56: level 2", [50.0, 60.0, 106.0, 116.0], 2),
    ("sqrt(area) = 28: level 1 clamped to 2 from below", [300.0, 40.0, 328.0, 68.0], 2),
    ("223 x 224: level 3", [32.0, 32.0, 255.0, 256.0], 3),
    ("sqrt(area) = 224 exactly: first size of level 4", [32.0, 32.0, 256.0, 256.0], 4),
    ("447 x 448: level 4", [16.0, 16.0, 463.0, 464.0], 4),
    ("sqrt(area) = 448 exactly: first size of level 5", [16.0, 16.0, 464.0, 464.0], 5),
    ("sqrt(area) = 896: level 6 clamped to 5 from above", [-192.0, -192.0, 704.0, 704.0], 5),
    ("zero area: every bin is the same point, level 2", [100.0, 100.0, 100.0, 100.0], 2),
]


def ka_coeffs(c=256):
    """per channel: f = a + 8 (level - 2) + 4 frame + bx * x + by * y on the level's pixel grid.  Every value is a multiple of 1/16 below
    128 -- 2 + 24 + 4 + 2 * (3 / 16) * 127 = 77.6 at most on the 128-pixel level-2 grid -- so the fp16 maps hold them exactly."""
    import numpy as np
    ch = np.arange(c)
    return (ch % 16) / 8.0, ((ch * 3) % 4) / 16.0, ((ch * 5 + 1) % 4) / 16.0


def ka_pyramid(n, c=256):
    import numpy as np
    a, bx, by = ka_coeffs(c)
    feats = []
    for l, s in enumerate(STRIDES4):
        h = w = KA_IMG // s
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        f = (a + 8.0 * l)[:, None, None] + bx[:, None, None] * xx[None] + by[:, None, None] * yy[None]
        feats.append(torch.from_numpy(np.stack([f + 4.0 * i for i in range(n)]).astype("float32")))
    return feats


def ka_boxes(n):
    return torch.tensor([[b for _, b, _ in KA_BOXES]] * n, dtype=torch.float32)


def ka_closed_form(n, c=256):
    """[n * M, C, 7, 7] float64: a sample at (y, x) contributes 0 when y < -1 or y > H or x < -1 or x > W and otherwise f(clamp(y), clamp(x));
    a bin is the mean of its 2 x 2 samples; level = clamp(floor(4 + log2(sqrt(area) / 224 + 1e-8)), 2, 5)"""
    import math
    import numpy as np
    a, bx, by = ka_coeffs(c)
    out = np.zeros((n * len(KA_BOXES), c, 7, 7))

    def clamp(t, L):
        if t <= 0:
            return 0.0
        return float(L - 1) if int(t) >= L - 1 else t
    for i in range(n):
        for j, (what, (x1, y1, x2, y2), level) in enumerate(KA_BOXES):
            lv = int(min(max(math.floor(4 + math.log2(math.sqrt((x2 - x1) * (y2 - y1)) / 224 + 1e-8)), 2), 5))
            assert lv == level, (what, lv)
            s = 1 << lv
            L = KA_IMG // s
            sx, sy = x1 / s - 0.5, y1 / s - 0.5
            bw, bh = (x2 / s - 0.5 - sx) / 7, (y2 / s - 0.5 - sy) / 7
            for ph in range(7):
                for pw in range(7):
                    acc = np.zeros(c)
                    for iy in range(2):
                        for ix in range(2):
                            y = sy + ph * bh + (iy + 0.5) * bh / 2
                            x = sx + pw * bw + (ix + 0.5) * bw / 2
                            if y < -1 or y > L or x < -1 or x > L:
                                continue
                            acc += a + 8.0 * (lv - 2) + 4.0 * i + bx * clamp(x, L) + by * clamp(y, L)
                    out[i * len(KA_BOXES) + j, :, ph, pw] = acc / 4
    return out
