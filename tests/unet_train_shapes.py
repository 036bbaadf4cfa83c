"""The batch shapes of tests/test_gpu_unet_train_shapes.py with what each is there for — TEST INFRASTRUCTURE.

Shared by the GPU module, which runs them, and tests/test_ut_gemm_plan_cpu.py, which proves from said_amd/csrc/ut_gemm_plan.h that a shape
reaches what it is named for.  Every weight gradient of the step at B x T runs K-split over K = B T in KS chunks of kchunk; `empty` says
whether the last chunk holds no k at all, `last` is the length of the last chunk that holds some.
"""
from collections import namedtuple

Shape = namedtuple("Shape", "B T KS kchunk empty last why")

#       B    T  KS kchunk empty last
DEFAULT = [
    Shape(1, 2, 1, 16, False, 2, "smallest admitted T, one sample"),
    Shape(3, 43, 1, 144, False, 129, "kchunk 144"),
    Shape(3, 86, 2, 144, False, 114, ""),
    Shape(3, 129, 3, 144, False, 99, "T % 64 = 1"),
    Shape(4, 130, 4, 144, False, 88, ""),
    Shape(5, 131, 5, 144, False, 79, "last tile 15 valid"),
    Shape(6, 133, 6, 144, False, 78, ""),
    Shape(8, 120, 7, 144, False, 96, "the benchmark's shape"),
    Shape(7, 147, 8, 144, False, 21, "last chunk 21 long"),
    Shape(9, 128, 9, 128, False, 128, "exact chunks"),
    Shape(7, 183, 10, 144, True, 129, "first empty chunk; the chunk before it ends with 1 valid k"),
    Shape(10, 141, 11, 144, True, 114, "empty chunk"),
    Shape(8, 197, 12, 144, True, 136, "empty chunk"),
    Shape(13, 130, 13, 144, True, 106, "empty chunk"),
    Shape(12, 150, 14, 144, True, 72, "empty chunk"),
    Shape(8, 240, 15, 128, False, 128, "the benchmark's other shape; exact chunks"),
    Shape(9, 228, 16, 144, True, 36, "empty chunk; last 36 long"),
    Shape(3, 683, 16, 144, True, 33, "longest rows: 11 softmax passes per lane; last tile 1 valid"),
    Shape(4, 600, 16, 160, True, 160, "kchunk 160: fifteen full chunks and an empty one; the headline clip length"),
]
MAX_BATCH, MAX_FRAMES = 13, 683       # the default context of the GPU module
VARIANTS = [(8, 120), (7, 183), (9, 228)]            # also with dropout, and with std + the vertex loss
ORDER = [(9, 228), (7, 183), (3, 43), (1, 2)]        # run in this order in one context
WIDE = (9, 228, 1024)                 # feature_dim = 1024: the projection's weight gradient fills the partial-tile buffer
FT_LAYERS = 2
FT_FULL = (9, 228)                    # fine-tuned encoder: the positional convolution's weight gradient fills the buffer
FT_SMALL = [(2, 128, 8), (1, 257, 1)]  # (B, T, KS of pos_fwd / pos_dgrad): M = 256 takes split_small, M = 257 does not
