"""The yardstick of the float16 / bfloat16 image outputs: the oracle's float32 output rounded once, to
nearest even, in numpy -- as 16-bit patterns."""
import numpy as np


def f16_bits(x):
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(over="ignore"):  # past 65504: +-inf, as the stage writes
        return x.astype(np.float16).view(np.uint16)


def bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def half_bits(x, name):
    return f16_bits(x) if name == "float16" else bf16_bits(x)
