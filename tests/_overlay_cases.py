"""The inputs of the overlay tests, built once and shared: tests/test_overlay.py checks them on the CPU (render_numpy against the painter
of _overlay_ref.py, and the conditions every random case has to meet), tests/test_gpu_overlay.py runs the kernels on the same inputs.
A case: frames (list of uint8 [h, w, 3]), dets fp32 [n, cap, 6] (model frame), counts int32 [n], ratios fp32 [n, 2], class_names,
atlas uint8 [95, gh, gw], threshold, thickness, text_scale.  Frames are a few tiles big: TILE = ops.OVERLAY_TILE = (64, 16)."""
import numpy as np

TILE = (64, 16)          # asserted equal to ops.OVERLAY_TILE in test_overlay.py
TW, TH = TILE
NAMES = ["bg", "cat", "a-name-of-24-bytes-xxxxx", "", "a name of more than twenty-four bytes", "café", "dog"]          # label 3: empty; 5: non-ASCII
NUM_CLASSES = len(NAMES) - 1
SHAPES = [(h, w) for h in (1, 37, 2 * TH + 1) for w in (53, 2 * TW + 1)]
SCORES = np.array([0.125, 0.375, 0.995, 0.705, 0.7, 0.71, 0.9, 0.9, 0.9, 0.85, 0.999, 1.0, 0.701], dtype=np.float32)


def pillow_atlas():
    from diffusionvid_amd.engine import demo
    return demo.glyph_atlas()


def random_atlas(seed=5, gh=9, gw=5):
    return (np.random.RandomState(seed).rand(95, gh, gw) < 0.4).astype(np.uint8)


def _garbage(rng, dets, counts):
    """rows at and beyond counts: NaN, infinities and huge values -- never read for meaning"""
    junk = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e9], dtype=np.float32)
    for f in range(dets.shape[0]):
        k = int(counts[f])
        dets[f, k:] = junk[rng.randint(0, len(junk), size=dets[f, k:].shape)]
    return dets


def random_case(seed, shapes, cap=24, threshold=0.7, thickness=2, text_scale=1, atlas=None, ratios=None):
    rng = np.random.RandomState(seed)
    n = len(shapes)
    frames = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in shapes]
    ratios = np.array(ratios if ratios is not None else [(rng.uniform(0.6, 1.9), rng.uniform(0.6, 1.9)) for _ in shapes], dtype=np.float64).astype(np.float32)
    dets = np.zeros((n, cap, 6), dtype=np.float32)
    counts = np.zeros((n,), dtype=np.int32)
    for f, (h, w) in enumerate(shapes):
        k = int(rng.randint(cap // 2, cap + 1))
        counts[f] = k
        x1 = rng.uniform(-12, w, k)
        y1 = rng.uniform(-12, h, k)
        bw = rng.uniform(-1, 0.8 * w + 8, k)
        bh = rng.uniform(-1, 0.8 * h + 8, k)
        d = np.stack([x1, y1, x1 + bw, y1 + bh], axis=1) / ratios[f][[0, 1, 0, 1]].astype(np.float64)
        dets[f, :k, :4] = d
        dets[f, :k, 4] = SCORES[rng.randint(0, len(SCORES), k)]
        dets[f, :k, 5] = rng.randint(0, NUM_CLASSES + 1, k)
    return dict(frames=frames, dets=_garbage(rng, dets, counts), counts=counts, ratios=ratios, class_names=NAMES, atlas=atlas if atlas is not None else pillow_atlas(),
                threshold=threshold, thickness=thickness, text_scale=text_scale)


def _case(frames_hw, rows_per_frame, seed=0, cap=None, counts=None, ratios=None, class_names=NAMES, **kw):
    """a hand-made case: rows_per_frame[f] = list of (x1, y1, x2, y2, score, label) in the native frame (ratio 1 unless given)"""
    rng = np.random.RandomState(1000 + seed)
    n = len(frames_hw)
    cap = cap or max(1, max(len(r) for r in rows_per_frame)) + 3
    dets = np.zeros((n, cap, 6), dtype=np.float32)
    cnt = np.array([len(r) for r in rows_per_frame] if counts is None else counts, dtype=np.int32)
    for f, rows in enumerate(rows_per_frame):
        if rows:
            dets[f, :len(rows)] = np.array(rows, dtype=np.float32)
    case = dict(frames=[rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in frames_hw], dets=_garbage(rng, dets, cnt), counts=cnt,
                ratios=np.array(ratios if ratios is not None else [(1.0, 1.0)] * n, dtype=np.float32), class_names=class_names, atlas=pillow_atlas(), threshold=0.7,
                thickness=2, text_scale=1)
    case.update(kw)
    return case


H2, W2 = 2 * TH + 1, 2 * TW + 1          # 33 x 129: three tiles on each axis


def geometry_case(thickness=2):
    """One 33 x 129 frame.  Rows, with what each is for (score rising, so this is also the draw order):"""
    nan, inf = float("nan"), float("inf")
    rows = [
        (TW - 4, TH - 4, TW + 6, TH + 5, 0.71, 1),          # 0 ring straddling the first tile edge on both axes
        (2 * TW - 1, 2 * TH - 1, 2 * TW, 2 * TH, 0.72, 6),          # 1 a 2 x 2 box on the second tile edge, ending on the frame's last pixel
        (300, 100, 340, 120, 0.73, 1),          # 2 wholly outside
        (-7, 8, 9, 14, 0.74, 2),          # 3 clipped at the left border, ring and plate
        (W2 - 9, 3, W2 + 30, 9, 0.75, 1),          # 4 clipped at the right border
        (20, -6, 40, 4, 0.76, 6),          # 5 clipped at the top
        (70, H2 - 4, 95, H2 + 12, 0.77, 1),          # 6 clipped at the bottom
        (W2 - 1, H2 - 1, W2 - 1, H2 - 1, 0.78, 6),          # 7 one pixel, the frame's last
        (50, 2, 50, 30, 0.79, 1),          # 8 x2 == x1
        (10.9, 5, 9.5, 20, 0.80, 1),          # 9 x2 < x1 after truncation: skipped
        (30, 20.2, 60, 19.9, 0.81, 1),          # 10 y2 < y1 after truncation: skipped
        (nan, 5, 30, 20, 0.82, 1),          # 11 not finite: skipped
        (5, 5, inf, 20, 0.83, 1),          # 12
        (5, 5, 30, 20, nan, 1),          # 13
        (5, 5, 30, 20, inf, 1),          # 14
        (-0.9, -0.9, 0.9, 0.9, 0.84, 6),          # 15 truncation toward zero: (0, 0, 0, 0), the frame's first pixel
        (100, 12, 112, 26, 0.7, 1),          # 16 the threshold itself: not drawn
    ]
    return _case([(H2, W2)], [rows], seed=1, thickness=thickness), [0, 1, 2, 3, 4, 5, 6, 7, 8, 15]


def empty_cases():
    rows = [(5, 5, 30, 20, 0.69, 1), (8, 2, 40, 30, 0.7, 2), (8, 2, 40, 30, float("nan"), 2)]
    return [_case([(37, 53), (H2, W2)], [[], []], seed=2, cap=4), _case([(37, 53), (H2, W2)], [rows, rows[:2]], seed=3),
            _case([(37, 53)], [rows], seed=4, counts=[0])]


def ties_case():
    """three equal scores with overlapping plates (drawn in row order), between a lower and a higher score given out of order"""
    rows = [(30, 12, 90, 30, 0.95, 1), (10, 4, 60, 20, 0.9, 6), (14, 8, 70, 25, 0.9, 1), (18, 12, 64, 28, 0.9, 2), (12, 6, 50, 22, 0.8, 6)]
    return _case([(H2, W2)], [rows], seed=5, cap=len(rows)), [4, 1, 2, 3, 0]          # counts == cap


def many_case():
    """300 passing rows at cap 300 (counts == cap): the last 256 in draw order are drawn; scores repeat, so the cut runs through ties"""
    rng = np.random.RandomState(77)
    k = 300
    x1, y1 = rng.uniform(-5, W2 - 8, k), rng.uniform(-5, H2 - 4, k)
    score = (0.71 + 0.001 * rng.randint(0, 40, k)).astype(np.float32)
    rows = [(x1[j], y1[j], x1[j] + rng.uniform(2, 40), y1[j] + rng.uniform(2, 16), score[j], rng.randint(0, NUM_CLASSES + 1)) for j in range(k)]
    order = sorted(range(k), key=lambda j: (float(score[j]), j))
    return _case([(H2, W2)], [rows], seed=6, cap=k), order[-256:]


def labels_case():
    """labels 0, num_classes + 1 and 1280 (no name beyond num_classes), the 24-byte name, the empty one, a name cut at 24 bytes, '?' bytes"""
    rows = [(4 + 18 * j, 2 + 3 * j, 30 + 18 * j, 14 + 3 * j, 0.75 + 0.01 * j, lab) for j, lab in enumerate((0, NUM_CLASSES + 1, 1280, 2, 3, 4, 5))]
    return _case([(H2, W2 + 60)], [rows], seed=7)


def thick_case(thickness, text_scale, atlas=None):
    """every thickness and text scale on one frame; row 1 is a 3 x 3 box, smaller than the larger thicknesses (a solid square)"""
    rows = [(20, 10, 100, 30, 0.8, 1), (70, 20, 72, 22, 0.9, 6), (TW - 2, TH - 2, TW + 40, TH + 12, 0.85, 2)]
    kw = dict(atlas=atlas) if atlas is not None else {}
    return _case([(H2, W2)], [rows], seed=8, thickness=thickness, text_scale=text_scale, **kw)


# seeds chosen on the CPU (test_overlay.py checks them): every case changes a ring pixel and a glyph pixel on each frame and has a pixel
# under two drawn detections
SCALE3_SEED = 25
SEEDS = {(1, 53): 21, (1, 2 * TW + 1): 31}          # one-row frames: most seeds leave no ring pixel in sight under the plates


def random_cases():
    cases = {"%dx%d" % hw: random_case(SEEDS.get(hw, 10), [hw]) for hw in SHAPES}
    cases["three sizes, one launch"] = random_case(13, [(37, 53), (H2, W2), (1, 53)])
    cases["random 5 x 9 atlas, scale 3, thickness 5"] = random_case(11, [(H2, W2)], atlas=random_atlas(), text_scale=3, thickness=5)
    cases["scale 3, thickness 1"] = random_case(SCALE3_SEED, [(37, 2 * TW + 1)], cap=6, text_scale=3, thickness=1)
    return cases
