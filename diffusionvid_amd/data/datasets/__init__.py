from .vid import VIDFrameList, VIDMEGATestDataset  # noqa: F401
from .still import OrientationBatchSampler, StillImageDataset, collate_images, orientation_batches  # noqa: F401
