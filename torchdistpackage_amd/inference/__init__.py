from .generate import (GraphedDecoder, GraphedGPT2Decoder,
                       GraphedLlamaDecoder, decode_forward, generate)
from ..ops.int8 import quantize_linears_

__all__ = ["generate", "decode_forward", "GraphedDecoder",
           "GraphedGPT2Decoder", "GraphedLlamaDecoder", "quantize_linears_"]
