from .generate import (GraphedGPT2Decoder, GraphedLlamaDecoder, generate)
from ..ops.int8 import quantize_linears_

__all__ = ["generate", "GraphedGPT2Decoder", "GraphedLlamaDecoder",
           "quantize_linears_"]
