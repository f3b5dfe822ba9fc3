from .dense import dense_assign, dense_sum  # noqa: F401
from .mx import mxfp8_dequantize, mxfp8_packed_nbytes, mxfp8_quantize  # noqa: F401
from .sparse import sparse_gather, sparse_scatter_add  # noqa: F401
