from .dense import dense_assign, dense_sum  # noqa: F401
from .mx import (mxfp8_dequantize, mxfp8_dequantize_many, mxfp8_packed_nbytes,  # noqa: F401
                 mxfp8_quantize, mxfp8_quantize_many)
from .sparse import sparse_gather, sparse_scatter_add  # noqa: F401
