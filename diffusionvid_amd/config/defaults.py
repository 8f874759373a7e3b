"""Config defaults for the DiffusionVID inference path.

Key names and default values follow the reference bit-for-bit for every key the hot path reads
(SURVEY.md 5 "Config"): mega_core/config/defaults.py (MODEL.VID.*, INPUT.*, DATALOADER.*, TEST.*)
and add_diffusiondet_config (mega_core/modeling/detector/diffusion_det.py:74-179).  Keys that only
serve training / other VOD methods are kept when the shipped YAMLs set them (so the reference's
YAML files parse unchanged) but nothing in this package reads them.
"""
from .node import CfgNode as CN

_C = CN()

_C.MODEL = CN()
_C.MODEL.DEVICE = "cuda"
_C.MODEL.META_ARCHITECTURE = "GeneralizedRCNN"
_C.MODEL.WEIGHT = ""
_C.MODEL.PIXEL_MEAN = [102.9801, 115.9465, 122.7717]
_C.MODEL.PIXEL_STD = [1.0, 1.0, 1.0]

_C.MODEL.BACKBONE = CN()
_C.MODEL.BACKBONE.CONV_BODY = "R-50-C4"
_C.MODEL.BACKBONE.NAME = "build_resnet_backbone"
_C.MODEL.BACKBONE.FREEZE_AT = 2
_C.MODEL.BACKBONE.FREEZE_CONV_BODY_AT = 2

_C.MODEL.RESNETS = CN()
_C.MODEL.RESNETS.DEPTH = 50
_C.MODEL.RESNETS.OUT_FEATURES = ["res4"]
_C.MODEL.RESNETS.NORM = "FrozenBN"
_C.MODEL.RESNETS.STRIDE_IN_1X1 = True
_C.MODEL.RESNETS.RES5_DILATION = 1
_C.MODEL.RESNETS.NUM_GROUPS = 1
_C.MODEL.RESNETS.WIDTH_PER_GROUP = 64
_C.MODEL.RESNETS.RES2_OUT_CHANNELS = 256
_C.MODEL.RESNETS.STEM_OUT_CHANNELS = 64
_C.MODEL.RESNETS.DEFORM_ON_PER_STAGE = (False, False, False, False)
_C.MODEL.RESNETS.DEFORM_MODULATED = False
_C.MODEL.RESNETS.DEFORM_NUM_GROUPS = 1

_C.MODEL.FPN = CN()
_C.MODEL.FPN.IN_FEATURES = []
_C.MODEL.FPN.OUT_CHANNELS = 256
_C.MODEL.FPN.NORM = ""
_C.MODEL.FPN.FUSE_TYPE = "sum"

_C.MODEL.RPN = CN()
_C.MODEL.RPN.ANCHOR_SIZES = (32, 64, 128, 256, 512)
_C.MODEL.RPN.PRE_NMS_TOP_N_TRAIN = 12000
_C.MODEL.RPN.PRE_NMS_TOP_N_TEST = 6000
_C.MODEL.RPN.POST_NMS_TOP_N_TRAIN = 2000
_C.MODEL.RPN.POST_NMS_TOP_N_TEST = 1000

_C.MODEL.ROI_HEADS = CN()
_C.MODEL.ROI_HEADS.IN_FEATURES = ["res4"]
_C.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 512
_C.MODEL.ROI_HEADS.SCORE_THRESH = 0.05
_C.MODEL.ROI_HEADS.NMS = 0.5
_C.MODEL.ROI_HEADS.DETECTIONS_PER_IMG = 100

_C.MODEL.ROI_BOX_HEAD = CN()
_C.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION = 14
_C.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO = 0
_C.MODEL.ROI_BOX_HEAD.POOLER_TYPE = "ROIAlignV2"
_C.MODEL.ROI_BOX_HEAD.NUM_CLASSES = 81

_C.MODEL.VID = CN()
_C.MODEL.VID.ENABLE = False
_C.MODEL.VID.METHOD = "base"
_C.MODEL.VID.RPN = CN()
_C.MODEL.VID.RPN.REF_PRE_NMS_TOP_N = 6000
_C.MODEL.VID.RPN.REF_POST_NMS_TOP_N = 75
_C.MODEL.VID.ROI_BOX_HEAD = CN()
_C.MODEL.VID.ROI_BOX_HEAD.ATTENTION = CN()
_C.MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE = False
_C.MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE = 3
_C.MODEL.VID.MEGA = CN()
_C.MODEL.VID.MEGA.MIN_OFFSET = -12
_C.MODEL.VID.MEGA.MAX_OFFSET = 12
_C.MODEL.VID.MEGA.ALL_FRAME_INTERVAL = 25
_C.MODEL.VID.MEGA.KEY_FRAME_LOCATION = 12
_C.MODEL.VID.MEGA.SHUFFLED_CUR_TEST = False
_C.MODEL.VID.MEGA.RATIO = 0.2
_C.MODEL.VID.MEGA.REF_NUM_LOCAL = 2
_C.MODEL.VID.MEGA.REF_NUM_GLOBAL = 2
_C.MODEL.VID.MEGA.MEMORY_MANAGEMENT_SIZE_TEST = 75
_C.MODEL.VID.MEGA.MEMORY_MANAGEMENT_SIZE_TRAIN = 75
_C.MODEL.VID.MEGA.MEMORY_MANAGEMENT_METRIC = "queue"
_C.MODEL.VID.MEGA.MEMORY_MANAGEMENT_TYPE = "greedy"
_C.MODEL.VID.MEGA.LOCAL = CN()
_C.MODEL.VID.MEGA.LOCAL.ENABLE = True
_C.MODEL.VID.MEGA.GLOBAL = CN()
_C.MODEL.VID.MEGA.GLOBAL.ENABLE = True
_C.MODEL.VID.MEGA.GLOBAL.RES_STAGE = 1
_C.MODEL.VID.MEGA.GLOBAL.SIZE = 10
_C.MODEL.VID.MEGA.GLOBAL.SHUFFLE = True
_C.MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST = False

_C.INPUT = CN()
_C.INPUT.MIN_SIZE_TRAIN = (800,)
_C.INPUT.MAX_SIZE_TRAIN = 1333
_C.INPUT.MIN_SIZE_TEST = 800
_C.INPUT.MAX_SIZE_TEST = 1333
_C.INPUT.PIXEL_MEAN = [102.9801, 115.9465, 122.7717]
_C.INPUT.PIXEL_STD = [1.0, 1.0, 1.0]
_C.INPUT.TO_BGR255 = True
_C.INPUT.TRANSFORM = False
_C.INPUT.INFER_BATCH = 1
# MI355X extension (not in the reference): number of INFER_BATCH groups whose backbone + feature-extraction heads are
# computed in ONE launch sequence.  1 = the reference's schedule.  > 1: the dataset hands the frames of the next
# LOOKAHEAD_BATCHES - 1 batches over early (item key "ref_ahead") and the detector keeps their per-frame results until
# the call that needs them; outputs are unchanged because those stages are per-frame independent.
_C.INPUT.LOOKAHEAD_BATCHES = 1

_C.DATASETS = CN()
_C.DATASETS.TRAIN = ()
_C.DATASETS.TEST = ()

_C.DATALOADER = CN()
_C.DATALOADER.NUM_WORKERS = 4
_C.DATALOADER.SIZE_DIVISIBILITY = 0

_C.SOLVER = CN(dict(
    OPTIMIZER_TYPE="sgd", LR_SCHEDULER_TYPE="step", BASE_LR=0.001, BIAS_LR_FACTOR=2.0, BACKBONE_MULTIPLIER=1.0,
    WEIGHT_DECAY=0.0005, WEIGHT_DECAY_BIAS=0.0, STEPS=(30000,), MAX_ITER=40000, WARMUP_ITERS=500, TEST_PERIOD=0,
    CHECKPOINT_PERIOD=2500, ACCUMULATION_STEPS=1, BATCH_REUSE_STEPS=1, IMS_PER_BATCH=16, OPTIMIZER="ADAMW"))

_C.TEST = CN()
_C.TEST.IMS_PER_BATCH = 8
_C.TEST.DETECTIONS_PER_IMG = 100
_C.TEST.SEQ_NMS = False
# test-time augmentation of still images (mega_core/config/defaults.py: TEST.BBOX_AUG, engine/bbox_aug.py): DiffusionDet.detect_images_aug
_C.TEST.BBOX_AUG = CN()
_C.TEST.BBOX_AUG.ENABLED = False
_C.TEST.BBOX_AUG.H_FLIP = False
_C.TEST.BBOX_AUG.SCALES = ()
_C.TEST.BBOX_AUG.MAX_SIZE = 4000
_C.TEST.BBOX_AUG.SCALE_H_FLIP = False

_C.OUTPUT_DIR = "."
_C.DTYPE = "float32"


def add_diffusiondet_config(cfg):
    """Keys of diffusion_det.py:74-179 (same names, same defaults)."""
    cfg.MODEL.DiffusionDet = CN()
    d = cfg.MODEL.DiffusionDet
    d.NUM_CLASSES = 80
    d.NUM_PROPOSALS = 300
    d.NHEADS = 8
    d.DROPOUT = 0.0
    d.DIM_FEEDFORWARD = 2048
    d.ACTIVATION = "relu"
    d.HIDDEN_DIM = 256
    d.NUM_CLS = 1
    d.NUM_REG = 3
    d.NUM_HEADS = 6
    d.NUM_HEADS_LOCAL = 0
    d.NUM_DYNAMIC = 2
    d.DIM_DYNAMIC = 64
    d.CLASS_WEIGHT = 2.0
    d.GIOU_WEIGHT = 2.0
    d.L1_WEIGHT = 5.0
    d.DEEP_SUPERVISION = True
    d.NO_OBJECT_WEIGHT = 0.1
    d.USE_FOCAL = True
    d.USE_FED_LOSS = False
    d.ALPHA = 0.25
    d.GAMMA = 2.0
    d.PRIOR_PROB = 0.01
    d.OTA_K = 5
    d.SNR_SCALE = 2.0
    d.SAMPLE_STEP = 1
    # MI355X extension: with SAMPLE_STEP > 1 skip the head passes whose outputs nothing reads -- the last
    # DDIM step (diffusion_det.py:573-575 `continue`s before the ensemble append) and the extraction heads on LOCAL frames
    # (their cached stages are only popped when SAMPLE_STEP == 1, box_head.py:300-302).  Detections are unchanged.
    d.SKIP_UNOBSERVABLE = False
    d.USE_NMS = True
    cfg.MODEL.SWIN = CN()
    cfg.MODEL.SWIN.SIZE = "B"
    cfg.MODEL.SWIN.USE_CHECKPOINT = False
    cfg.MODEL.SWIN.OUT_FEATURES = (0, 1, 2, 3)
    cfg.MODEL.PIXEL_MEAN = [123.675, 116.280, 103.530]
    cfg.MODEL.PIXEL_STD = [58.395, 57.120, 57.375]
    cfg.MODEL.BACKBONE.NAME = "build_resnet_backbone"
    cfg.MODEL.BACKBONE.FREEZE_AT = 2
    cfg.MODEL.RESNETS.OUT_FEATURES = ["res2", "res3", "res4", "res5"]
    cfg.MODEL.FPN.IN_FEATURES = ["res2", "res3", "res4", "res5"]
    cfg.MODEL.FPN.OUT_CHANNELS = 256
    cfg.MODEL.ROI_HEADS.IN_FEATURES = ["p2", "p3", "p4", "p5"]
    cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE = "ROIAlignV2"
    cfg.MODEL.RESNETS.NORM = "FrozenBN"
    cfg.MODEL.RESNETS.DEPTH = 101
    cfg.MODEL.RESNETS.STRIDE_IN_1X1 = False
    cfg.SOLVER.CLIP_GRADIENTS = CN(dict(ENABLED=True, CLIP_TYPE="full_model", CLIP_VALUE=1.0, NORM_TYPE=2.0))
    cfg.INPUT.TO_BGR255 = False
    cfg.INPUT.INFER_BATCH = 1
