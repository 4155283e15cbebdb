"""The WebP writer's contract restated in numpy / pure Python: a VP8 key-frame encoder of exactly the subset that
csrc/webp.hip + webpcode.py write, and what libwebp shows for its files.  The tests hold the device code to these bytes and hold
this text to libwebp (Pillow) on every decoded byte.  The tables are the format's constants (RFC 6386)."""
import math
import struct

import numpy as np

# default coefficient probabilities [block type 4][band 8][context 3][node 11]
COEFF_PROBS = [
    128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128,
    253, 136, 254, 255, 228, 219, 128, 128, 128, 128, 128, 189, 129, 242, 255, 227, 213, 255, 219, 128, 128, 128, 106, 126, 227, 252, 214, 209, 255, 255, 128, 128, 128,
    1, 98, 248, 255, 236, 226, 255, 255, 128, 128, 128, 181, 133, 238, 254, 221, 234, 255, 154, 128, 128, 128, 78, 134, 202, 247, 198, 180, 255, 219, 128, 128, 128,
    1, 185, 249, 255, 243, 255, 128, 128, 128, 128, 128, 184, 150, 247, 255, 236, 224, 128, 128, 128, 128, 128, 77, 110, 216, 255, 236, 230, 128, 128, 128, 128, 128,
    1, 101, 251, 255, 241, 255, 128, 128, 128, 128, 128, 170, 139, 241, 252, 236, 209, 255, 255, 128, 128, 128, 37, 116, 196, 243, 228, 255, 255, 255, 128, 128, 128,
    1, 204, 254, 255, 245, 255, 128, 128, 128, 128, 128, 207, 160, 250, 255, 238, 128, 128, 128, 128, 128, 128, 102, 103, 231, 255, 211, 171, 128, 128, 128, 128, 128,
    1, 152, 252, 255, 240, 255, 128, 128, 128, 128, 128, 177, 135, 243, 255, 234, 225, 128, 128, 128, 128, 128, 80, 129, 211, 255, 194, 224, 128, 128, 128, 128, 128,
    1, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128, 246, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128, 255, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128,
    198, 35, 237, 223, 193, 187, 162, 160, 145, 155, 62, 131, 45, 198, 221, 172, 176, 220, 157, 252, 221, 1, 68, 47, 146, 208, 149, 167, 221, 162, 255, 223, 128,
    1, 149, 241, 255, 221, 224, 255, 255, 128, 128, 128, 184, 141, 234, 253, 222, 220, 255, 199, 128, 128, 128, 81, 99, 181, 242, 176, 190, 249, 202, 255, 255, 128,
    1, 129, 232, 253, 214, 197, 242, 196, 255, 255, 128, 99, 121, 210, 250, 201, 198, 255, 202, 128, 128, 128, 23, 91, 163, 242, 170, 187, 247, 210, 255, 255, 128,
    1, 200, 246, 255, 234, 255, 128, 128, 128, 128, 128, 109, 178, 241, 255, 231, 245, 255, 255, 128, 128, 128, 44, 130, 201, 253, 205, 192, 255, 255, 128, 128, 128,
    1, 132, 239, 251, 219, 209, 255, 165, 128, 128, 128, 94, 136, 225, 251, 218, 190, 255, 255, 128, 128, 128, 22, 100, 174, 245, 186, 161, 255, 199, 128, 128, 128,
    1, 182, 249, 255, 232, 235, 128, 128, 128, 128, 128, 124, 143, 241, 255, 227, 234, 128, 128, 128, 128, 128, 35, 77, 181, 251, 193, 211, 255, 205, 128, 128, 128,
    1, 157, 247, 255, 236, 231, 255, 255, 128, 128, 128, 121, 141, 235, 255, 225, 227, 255, 255, 128, 128, 128, 45, 99, 188, 251, 195, 217, 255, 224, 128, 128, 128,
    1, 1, 251, 255, 213, 255, 128, 128, 128, 128, 128, 203, 1, 248, 255, 255, 128, 128, 128, 128, 128, 128, 137, 1, 177, 255, 224, 255, 128, 128, 128, 128, 128,
    253, 9, 248, 251, 207, 208, 255, 192, 128, 128, 128, 175, 13, 224, 243, 193, 185, 249, 198, 255, 255, 128, 73, 17, 171, 221, 161, 179, 236, 167, 255, 234, 128,
    1, 95, 247, 253, 212, 183, 255, 255, 128, 128, 128, 239, 90, 244, 250, 211, 209, 255, 255, 128, 128, 128, 155, 77, 195, 248, 188, 195, 255, 255, 128, 128, 128,
    1, 24, 239, 251, 218, 219, 255, 205, 128, 128, 128, 201, 51, 219, 255, 196, 186, 128, 128, 128, 128, 128, 69, 46, 190, 239, 201, 218, 255, 228, 128, 128, 128,
    1, 191, 251, 255, 255, 128, 128, 128, 128, 128, 128, 223, 165, 249, 255, 213, 255, 128, 128, 128, 128, 128, 141, 124, 248, 255, 255, 128, 128, 128, 128, 128, 128,
    1, 16, 248, 255, 255, 128, 128, 128, 128, 128, 128, 190, 36, 230, 255, 236, 255, 128, 128, 128, 128, 128, 149, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128,
    1, 226, 255, 128, 128, 128, 128, 128, 128, 128, 128, 247, 192, 255, 128, 128, 128, 128, 128, 128, 128, 128, 240, 128, 255, 128, 128, 128, 128, 128, 128, 128, 128,
    1, 134, 252, 255, 255, 128, 128, 128, 128, 128, 128, 213, 62, 250, 255, 255, 128, 128, 128, 128, 128, 128, 55, 93, 255, 128, 128, 128, 128, 128, 128, 128, 128,
    128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128,
    202, 24, 213, 235, 186, 191, 220, 160, 240, 175, 255, 126, 38, 182, 232, 169, 184, 228, 174, 255, 187, 128, 61, 46, 138, 219, 151, 178, 240, 170, 255, 216, 128,
    1, 112, 230, 250, 199, 191, 247, 159, 255, 255, 128, 166, 109, 228, 252, 211, 215, 255, 174, 128, 128, 128, 39, 77, 162, 232, 172, 180, 245, 178, 255, 255, 128,
    1, 52, 220, 246, 198, 199, 249, 220, 255, 255, 128, 124, 74, 191, 243, 183, 193, 250, 221, 255, 255, 128, 24, 71, 130, 219, 154, 170, 243, 182, 255, 255, 128,
    1, 182, 225, 249, 219, 240, 255, 224, 128, 128, 128, 149, 150, 226, 252, 216, 205, 255, 171, 128, 128, 128, 28, 108, 170, 242, 183, 194, 254, 223, 255, 255, 128,
    1, 81, 230, 252, 204, 203, 255, 192, 128, 128, 128, 123, 102, 209, 247, 188, 196, 255, 233, 128, 128, 128, 20, 95, 153, 243, 164, 173, 255, 203, 128, 128, 128,
    1, 222, 248, 255, 216, 213, 128, 128, 128, 128, 128, 168, 175, 246, 252, 235, 205, 255, 255, 128, 128, 128, 47, 116, 215, 255, 211, 212, 255, 255, 128, 128, 128,
    1, 121, 236, 253, 212, 214, 255, 255, 128, 128, 128, 141, 84, 213, 252, 201, 202, 255, 219, 128, 128, 128, 42, 80, 160, 240, 162, 185, 255, 205, 128, 128, 128,
    1, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128, 244, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128, 238, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128]
# the probabilities of the "update this coefficient probability" flags, same shape
COEFF_UPDATE_PROBS = [
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    176, 246, 255, 255, 255, 255, 255, 255, 255, 255, 255, 223, 241, 252, 255, 255, 255, 255, 255, 255, 255, 255, 249, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 244, 252, 255, 255, 255, 255, 255, 255, 255, 255, 234, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 253, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 246, 254, 255, 255, 255, 255, 255, 255, 255, 255, 239, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 248, 254, 255, 255, 255, 255, 255, 255, 255, 255, 251, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 251, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 254, 253, 255, 254, 255, 255, 255, 255, 255, 255, 250, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    217, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 225, 252, 241, 253, 255, 255, 254, 255, 255, 255, 255, 234, 250, 241, 250, 253, 255, 253, 254, 255, 255, 255,
    255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 223, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 238, 253, 254, 254, 255, 255, 255, 255, 255, 255, 255,
    255, 248, 254, 255, 255, 255, 255, 255, 255, 255, 255, 249, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 253, 255, 255, 255, 255, 255, 255, 255, 255, 255, 247, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 252, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 253, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 254, 253, 255, 255, 255, 255, 255, 255, 255, 255, 250, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    186, 251, 250, 255, 255, 255, 255, 255, 255, 255, 255, 234, 251, 244, 254, 255, 255, 255, 255, 255, 255, 255, 251, 251, 243, 253, 254, 255, 254, 255, 255, 255, 255,
    255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 236, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 251, 253, 253, 254, 254, 255, 255, 255, 255, 255, 255,
    255, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 254, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    248, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 250, 254, 252, 254, 255, 255, 255, 255, 255, 255, 255, 248, 254, 249, 253, 255, 255, 255, 255, 255, 255, 255,
    255, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255, 246, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255, 252, 254, 251, 254, 254, 255, 255, 255, 255, 255, 255,
    255, 254, 252, 255, 255, 255, 255, 255, 255, 255, 255, 248, 254, 253, 255, 255, 255, 255, 255, 255, 255, 255, 253, 255, 254, 254, 255, 255, 255, 255, 255, 255, 255,
    255, 251, 254, 255, 255, 255, 255, 255, 255, 255, 255, 245, 251, 254, 255, 255, 255, 255, 255, 255, 255, 255, 253, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 251, 253, 255, 255, 255, 255, 255, 255, 255, 255, 252, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 252, 255, 255, 255, 255, 255, 255, 255, 255, 255, 249, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 253, 255, 255, 255, 255, 255, 255, 255, 255, 250, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255]
# quantiser steps by index
DC_TABLE = [
    4, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13, 14, 15, 16, 17, 17, 18, 19, 20, 20, 21, 21, 22, 22, 23, 23, 24, 25, 25, 26, 27, 28,
    29, 30, 31, 32, 33, 34, 35, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58,
    59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 76, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89,
    91, 93, 95, 96, 98, 100, 101, 102, 104, 106, 108, 110, 112, 114, 116, 118, 122, 124, 126, 128, 130, 132, 134, 136, 138, 140, 143, 145, 148, 151, 154, 157]
AC_TABLE = [
    4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35,
    36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 60, 62, 64, 66, 68, 70, 72, 74, 76,
    78, 80, 82, 84, 86, 88, 90, 92, 94, 96, 98, 100, 102, 104, 106, 108, 110, 112, 114, 116, 119, 122, 125, 128, 131, 134, 137, 140, 143, 146, 149, 152,
    155, 158, 161, 164, 167, 170, 173, 177, 181, 185, 189, 193, 197, 201, 205, 209, 213, 217, 221, 225, 229, 234, 239, 245, 249, 254, 259, 264, 269, 274, 279, 284]

ZIGZAG = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]
BANDS = [0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0]
CAT3, CAT4, CAT5 = [173, 148, 140], [176, 155, 140, 135], [180, 157, 141, 134, 130]
CAT6 = [254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129]
YMODE_PROBS = (145, 156, 163, 128)         # key-frame luma mode tree: B_PRED | (DC | V) | (H | TM)
UVMODE_PROBS = (142, 114, 183)             # chroma mode tree: DC | V | (H | TM)
DC_PRED, V_PRED, H_PRED, TM_PRED = 0, 1, 2, 3
MAX_LEVEL = 2047
MAX_SIDE = 16383

PROBS = np.array(COEFF_PROBS, np.int64).reshape(4, 8, 3, 11).tolist()


# ---- the boolean (arithmetic) coder -------------------------------------------------------------------------------------------
class BoolEncoder:
    """The format's boolean coder in its byte-wise form: `range` holds the range minus one (127..254 between calls), `value` the
    low end, `nb_bits` the bits of `value` past the next whole byte (-8 at the start).  A finished byte is held back while it may
    still take a carry: the last byte that is not 0xFF as out[-1], the 0xFF bytes behind it as the count `run`."""

    def __init__(self):
        self.range, self.value, self.run, self.nb_bits, self.out = 254, 0, 0, -8, bytearray()

    def put(self, prob, bit):
        split = (self.range * prob) >> 8
        if bit:
            self.value += split + 1
            self.range -= split + 1
        else:
            self.range = split
        if self.range < 127:
            shift = 8 - (self.range + 1).bit_length()
            self.range = ((self.range + 1) << shift) - 1
            self.value <<= shift
            self.nb_bits += shift
            if self.nb_bits > 0:
                self._flush()

    def put_bits(self, value, n):
        for k in range(n - 1, -1, -1):
            self.put(128, (value >> k) & 1)

    def _flush(self):
        s = 8 + self.nb_bits
        bits = self.value >> s
        self.value -= bits << s
        self.nb_bits -= 8
        if (bits & 0xFF) != 0xFF:
            carry = bits >> 8
            if carry and self.out:
                self.out[-1] += 1
            self.out += bytes([0x00 if carry else 0xFF]) * self.run
            self.run = 0
            self.out.append(bits & 0xFF)
        else:
            assert bits == 0xFF
            self.run += 1

    def finish(self):
        self.put_bits(0, 9 - self.nb_bits)
        self.nb_bits = 0
        self._flush()
        self.out += b'\xFF' * self.run
        self.run = 0
        return bytes(self.out)


def code_pairs(pairs):
    """the bytes of a sequence of (probability, bit) pairs"""
    e = BoolEncoder()
    for p, b in pairs:
        e.put(p, b)
    return e.finish()


# ---- colour ------------------------------------------------------------------------------------------------------------------
def quality_to_qi(quality):
    """quality 100..1 onto the quantiser index 0..127"""
    return ((100 - quality) * 127 + 49) // 99


def filter_level(qi):
    return qi >> 2


def quantisers(qi):
    """(dc, ac) steps of Y, Y2 and chroma for the frame's one quantiser index (all deltas 0)"""
    dc, ac = DC_TABLE[qi], AC_TABLE[qi]
    return (dc, ac), (2 * dc, max(8, ac * 155 // 100)), (min(dc, 132), ac)


def planes_of(frame):
    """BGR uint8 [H,W,3] -> (Y [Hp,Wp], U, V [Hp/2,Wp/2]) as int64; Hp, Wp the next multiples of 16, the right and bottom edges
    replicated before the conversion.  Y of a pixel, Cb and Cr of the sums over a 2x2 cell, BT.601 studio range in 16 / 18
    fraction bits with round-half-up."""
    H, W = frame.shape[:2]
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    f = np.pad(frame.astype(np.int64), ((0, Hp - H), (0, Wp - W), (0, 0)), mode='edge')
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = (16839 * r + 33059 * g + 6420 * b + 1081344) >> 16
    s = f.reshape(Hp // 2, 2, Wp // 2, 2, 3).sum(axis=(1, 3))
    b, g, r = s[..., 0], s[..., 1], s[..., 2]
    u = (-9719 * r - 19081 * g + 28800 * b + 33685504) >> 18
    v = (28800 * r - 24116 * g - 4684 * b + 33685504) >> 18
    return np.clip(y, 0, 255), np.clip(u, 0, 255), np.clip(v, 0, 255)


# ---- transforms ---------------------------------------------------------------------------------------------------------------
def fdct(d):
    """forward 4x4 transform (ours): d [k,4,4] residuals (row, column) -> [k,16] coefficients, 4 * vertical + horizontal frequency"""
    a0, a1, a2, a3 = d[:, :, 0] + d[:, :, 3], d[:, :, 1] + d[:, :, 2], d[:, :, 1] - d[:, :, 2], d[:, :, 0] - d[:, :, 3]
    t = np.stack([(a0 + a1) * 8, (a2 * 2217 + a3 * 5352 + 1812) >> 9, (a0 - a1) * 8, (a3 * 2217 - a2 * 5352 + 937) >> 9], axis=2)
    a0, a1, a2, a3 = t[:, 0] + t[:, 3], t[:, 1] + t[:, 2], t[:, 1] - t[:, 2], t[:, 0] - t[:, 3]
    o = np.stack([(a0 + a1 + 7) >> 4, ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0), (a0 - a1 + 7) >> 4,
                  (a3 * 2217 - a2 * 5352 + 51000) >> 16], axis=1)
    return o.reshape(-1, 16)


def _mul1(a):
    return ((a * 20091) >> 16) + a


def _mul2(a):
    return (a * 35468) >> 16


def idct(c):
    """the format's inverse 4x4 transform: c [k,16] -> [k,4,4] residuals (row, column), before the add to the prediction"""
    c = c.reshape(-1, 4, 4)
    a, b = c[:, 0] + c[:, 2], c[:, 0] - c[:, 2]
    cc, d = _mul2(c[:, 1]) - _mul1(c[:, 3]), _mul1(c[:, 1]) + _mul2(c[:, 3])
    t = np.stack([a + d, b + cc, b - cc, a - d], axis=1)             # [k, row, column]
    dc = t[:, :, 0] + 4
    a, b = dc + t[:, :, 2], dc - t[:, :, 2]
    cc, d = _mul2(t[:, :, 1]) - _mul1(t[:, :, 3]), _mul1(t[:, :, 1]) + _mul2(t[:, :, 3])
    return np.stack([(a + d) >> 3, (b + cc) >> 3, (b - cc) >> 3, (a - d) >> 3], axis=2)


def fwht(v):
    """forward Walsh-Hadamard transform (ours) of the 16 luma DCs (4 * block row + block column)"""
    v = v.reshape(4, 4)
    a0, a1, a2, a3 = v[:, 0] + v[:, 2], v[:, 1] + v[:, 3], v[:, 1] - v[:, 3], v[:, 0] - v[:, 2]
    t = np.stack([a0 + a1, a3 + a2, a3 - a2, a0 - a1], axis=1)
    a0, a1, a2, a3 = t[0] + t[2], t[1] + t[3], t[1] - t[3], t[0] - t[2]
    return (np.stack([a0 + a1, a3 + a2, a3 - a2, a0 - a1]) >> 1).reshape(16)


def iwht(v):
    """the format's inverse Walsh-Hadamard transform: 16 Y2 coefficients -> the DC of the 16 luma blocks"""
    v = v.reshape(4, 4)
    a0, a1, a2, a3 = v[0] + v[3], v[1] + v[2], v[1] - v[2], v[0] - v[3]
    t = np.stack([a0 + a1, a3 + a2, a0 - a1, a3 - a2])
    dc = t[:, 0] + 3
    a0, a1, a2, a3 = dc + t[:, 3], t[:, 1] + t[:, 2], t[:, 1] - t[:, 2], dc - t[:, 3]
    return np.stack([(a0 + a1) >> 3, (a3 + a2) >> 3, (a0 - a1) >> 3, (a3 - a2) >> 3], axis=1).reshape(16)


def quantise(c, dcq, acq):
    """c [...,16] -> levels: (|c| + bias) // q with the sign of c, bias q >> 1 for index 0 and 3 * q >> 3 for the others,
    clamped to MAX_LEVEL"""
    q = np.full(16, acq, np.int64)
    q[0] = dcq
    bias = (3 * q) >> 3
    bias[0] = dcq >> 1
    lev = np.minimum((np.abs(c) + bias) // q, MAX_LEVEL)
    return np.where(c < 0, -lev, lev), q


# ---- prediction ---------------------------------------------------------------------------------------------------------------
def predictions(rec, mbx, mby, size):
    """the four predictions [4,size,size] (DC, V, H, TM) of the block at macroblock (mbx, mby) of the reconstructed plane `rec`"""
    x0, y0 = mbx * size, mby * size
    top = rec[y0 - 1, x0:x0 + size] if mby else np.full(size, 127, np.int64)
    left = rec[y0:y0 + size, x0 - 1] if mbx else np.full(size, 129, np.int64)
    tl = rec[y0 - 1, x0 - 1] if (mbx and mby) else (129 if mby else 127)
    sh = 3 if size == 8 else 4
    if mbx and mby:
        dc = (top.sum() + left.sum() + size) >> (sh + 1)
    elif mby:
        dc = (top.sum() + (size >> 1)) >> sh
    elif mbx:
        dc = (left.sum() + (size >> 1)) >> sh
    else:
        dc = 128
    return np.stack([np.full((size, size), dc, np.int64), np.broadcast_to(top, (size, size)),
                     np.broadcast_to(left[:, None], (size, size)), np.clip(left[:, None] + top[None, :] - tl, 0, 255)])


def _blocks(a):
    """[4k,4k] -> [k*k,4,4], blocks in raster order"""
    k = a.shape[0] // 4
    return a.reshape(k, 4, k, 4).transpose(0, 2, 1, 3).reshape(k * k, 4, 4)


def _unblocks(b):
    k = int(round(b.shape[0] ** 0.5))
    return b.reshape(k, k, 4, 4).transpose(0, 2, 1, 3).reshape(4 * k, 4 * k)


# ---- tokens -------------------------------------------------------------------------------------------------------------------
def block_pairs(levels, first, kind, ctx, out):
    """append the (probability, bit) pairs of one block's 16 zigzag-ordered levels, coded from position `first` with the
    probabilities of block type `kind` and the context `ctx`; returns 1 if the block has a non-zero level, else 0"""
    last = -1
    for i in range(15, first - 1, -1):
        if levels[i]:
            last = i
            break
    n = first
    p = PROBS[kind][BANDS[n]][int(ctx)]
    out.append((p[0], int(last >= 0)))
    if last < 0:
        return 0
    while n < 16:
        c = int(levels[n])
        n += 1
        v = abs(c)
        out.append((p[1], int(v != 0)))
        if v == 0:
            p = PROBS[kind][BANDS[n]][0]
            continue
        out.append((p[2], int(v > 1)))
        if v == 1:
            p = PROBS[kind][BANDS[n]][1]
        else:
            out.append((p[3], int(v > 4)))
            if v <= 4:
                out.append((p[4], int(v != 2)))
                if v != 2:
                    out.append((p[5], int(v == 4)))
            else:
                out.append((p[6], int(v > 10)))
                if v <= 10:
                    out.append((p[7], int(v > 6)))
                    if v <= 6:
                        out.append((159, int(v == 6)))
                    else:
                        out.append((165, int(v >= 9)))
                        out.append((145, int(not v & 1)))
                else:
                    if v < 3 + (8 << 1):
                        out += [(p[8], 0), (p[9], 0)]
                        v, tab = v - (3 + (8 << 0)), CAT3
                    elif v < 3 + (8 << 2):
                        out += [(p[8], 0), (p[9], 1)]
                        v, tab = v - (3 + (8 << 1)), CAT4
                    elif v < 3 + (8 << 3):
                        out += [(p[8], 1), (p[10], 0)]
                        v, tab = v - (3 + (8 << 2)), CAT5
                    else:
                        out += [(p[8], 1), (p[10], 1)]
                        v, tab = v - (3 + (8 << 3)), CAT6
                    for k, pr in enumerate(tab):
                        out.append((pr, (v >> (len(tab) - 1 - k)) & 1))
            p = PROBS[kind][BANDS[n]][2]
        out.append((128, int(c < 0)))
        if n == 16:
            return 1
        out.append((p[0], int(n <= last)))
        if n > last:
            return 1
    return 1


# ---- one frame ------------------------------------------------------------------------------------------------------------------
def encode_frame(frame, quality=90):
    """One BGR uint8 frame [H,W,3] -> dict: 'vp8' the VP8 key frame (frame header, first partition, partition sizes, token
    partitions), 'ymodes' and 'uvmodes' [mbh,mbw], 'planes' the reconstruction (Y, U, V) before any loop filter, 'inner' [mbh,mbw]
    whether a decoder filters the macroblock's inner edges, 'level' the loop-filter level, 'first' and 'parts' the partitions."""
    H, W = frame.shape[:2]
    assert frame.dtype == np.uint8 and frame.shape[2] == 3 and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE
    qi = quality_to_qi(quality)
    (y1dc, y1ac), (y2dc, y2ac), (uvdc, uvac) = quantisers(qi)
    src = planes_of(frame)
    mbh, mbw = src[0].shape[0] // 16, src[0].shape[1] // 16
    rec = [np.zeros_like(p) for p in src]
    ymodes, uvmodes = np.zeros((mbh, mbw), np.int64), np.zeros((mbh, mbw), np.int64)
    inner = np.zeros((mbh, mbw), bool)
    skip = np.zeros((mbh, mbw), bool)
    lev_y2 = np.zeros((mbh, mbw, 16), np.int64)                      # zigzag order from here on
    lev_y = np.zeros((mbh, mbw, 16, 16), np.int64)
    lev_c = np.zeros((2, mbh, mbw, 4, 16), np.int64)
    for mby in range(mbh):
        for mbx in range(mbw):
            ys, xs = slice(16 * mby, 16 * mby + 16), slice(16 * mbx, 16 * mbx + 16)
            preds = predictions(rec[0], mbx, mby, 16)
            sse = ((preds - src[0][ys, xs]) ** 2).sum(axis=(1, 2))
            m = int(np.argmin(sse))                                  # the first of equal minima: the lower mode number
            ymodes[mby, mbx] = m
            coef = fdct(_blocks(src[0][ys, xs] - preds[m]))
            l2, q2 = quantise(fwht(coef[:, 0]), y2dc, y2ac)
            dcs = iwht(l2 * q2)
            ly, qy = quantise(coef, y1ac, y1ac)
            ly[:, 0] = 0
            deq = ly * qy
            deq[:, 0] = dcs
            rec[0][ys, xs] = np.clip(preds[m] + _unblocks(idct(deq)), 0, 255)
            lev_y2[mby, mbx] = l2[ZIGZAG]
            lev_y[mby, mbx] = ly[:, ZIGZAG]
            ys, xs = slice(8 * mby, 8 * mby + 8), slice(8 * mbx, 8 * mbx + 8)
            pu, pv = predictions(rec[1], mbx, mby, 8), predictions(rec[2], mbx, mby, 8)
            sse = ((pu - src[1][ys, xs]) ** 2).sum(axis=(1, 2)) + ((pv - src[2][ys, xs]) ** 2).sum(axis=(1, 2))
            m = int(np.argmin(sse))
            uvmodes[mby, mbx] = m
            for c, pred in ((0, pu[m]), (1, pv[m])):
                lc, qc = quantise(fdct(_blocks(src[1 + c][ys, xs] - pred)), uvdc, uvac)
                rec[1 + c][ys, xs] = np.clip(pred + _unblocks(idct(lc * qc)), 0, 255)
                lev_c[c, mby, mbx] = lc[:, ZIGZAG]
            skip[mby, mbx] = not (l2.any() or ly.any() or lev_c[:, mby, mbx].any())
            inner[mby, mbx] = bool(ly.any() or dcs.any() or lev_c[:, mby, mbx].any())
    # token partitions: macroblock row r goes to partition r % parts
    log2parts = min(3, mbh.bit_length() - 1)
    nparts = 1 << log2parts
    pairs = [[] for _ in range(nparts)]
    top_y, top_c, top_y2 = np.zeros(4 * mbw, np.int64), np.zeros((2, 2 * mbw), np.int64), np.zeros(mbw, np.int64)
    for mby in range(mbh):
        out = pairs[mby % nparts]
        left_y, left_c, left_y2 = np.zeros(4, np.int64), np.zeros((2, 2), np.int64), 0
        for mbx in range(mbw):
            if skip[mby, mbx]:
                left_y[:], left_c[:], left_y2 = 0, 0, 0
                top_y[4 * mbx:4 * mbx + 4], top_c[:, 2 * mbx:2 * mbx + 2], top_y2[mbx] = 0, 0, 0
                continue
            left_y2 = top_y2[mbx] = block_pairs(lev_y2[mby, mbx], 0, 1, left_y2 + top_y2[mbx], out)
            for by in range(4):
                for bx in range(4):
                    nz = block_pairs(lev_y[mby, mbx, 4 * by + bx], 1, 0, left_y[by] + top_y[4 * mbx + bx], out)
                    left_y[by] = top_y[4 * mbx + bx] = nz
            for c in range(2):
                for by in range(2):
                    for bx in range(2):
                        nz = block_pairs(lev_c[c, mby, mbx, 2 * by + bx], 0, 2, left_c[c, by] + top_c[c, 2 * mbx + bx], out)
                        left_c[c, by] = top_c[c, 2 * mbx + bx] = nz
    parts = [code_pairs(p) for p in pairs]
    # first partition
    total, nskip = mbh * mbw, int(skip.sum())
    prob_skip = max(1, (total - nskip) * 255 // total)
    level = filter_level(qi)
    e = BoolEncoder()
    e.put_bits(0, 1)                  # colour space
    e.put_bits(0, 1)                  # clamping needed
    e.put_bits(0, 1)                  # no segmentation
    e.put_bits(1, 1)                  # simple loop filter
    e.put_bits(level, 6)
    e.put_bits(0, 3)                  # sharpness
    e.put_bits(0, 1)                  # no filter deltas
    e.put_bits(log2parts, 2)
    e.put_bits(qi, 7)
    e.put_bits(0, 5)                  # no quantiser deltas
    e.put_bits(0, 1)                  # refresh_entropy_probs
    for p in COEFF_UPDATE_PROBS:
        e.put(p, 0)                   # no probability update
    e.put_bits(1, 1)                  # mb_no_coeff_skip
    e.put_bits(prob_skip, 8)
    for mby in range(mbh):
        for mbx in range(mbw):
            e.put(prob_skip, int(skip[mby, mbx]))
            m = int(ymodes[mby, mbx])
            e.put(YMODE_PROBS[0], 1)                                 # not B_PRED
            e.put(YMODE_PROBS[1], m >> 1)
            e.put(YMODE_PROBS[3] if m >> 1 else YMODE_PROBS[2], m & 1)
            m = int(uvmodes[mby, mbx])
            e.put(UVMODE_PROBS[0], int(m != DC_PRED))
            if m != DC_PRED:
                e.put(UVMODE_PROBS[1], int(m != V_PRED))
                if m != V_PRED:
                    e.put(UVMODE_PROBS[2], int(m == TM_PRED))
    first = e.finish()
    return {'vp8': vp8_frame(first, parts, W, H), 'first': first, 'parts': parts, 'ymodes': ymodes, 'uvmodes': uvmodes,
            'planes': tuple(rec), 'inner': inner, 'level': level, 'skip': skip}


# ---- containers -----------------------------------------------------------------------------------------------------------------
def vp8_frame(first, parts, width, height):
    """frame tag (key frame, version 1, shown, the first partition's size), start code, size, first partition, the sizes of all
    token partitions but the last in 3 bytes each, the token partitions"""
    assert len(first) < 1 << 19 and all(len(p) < 1 << 24 for p in parts)
    tag = 0 | 1 << 1 | 1 << 4 | len(first) << 5
    head = struct.pack('<I', tag)[:3] + b'\x9d\x01\x2a' + struct.pack('<HH', width, height)
    return head + first + b''.join(struct.pack('<I', len(p))[:3] for p in parts[:-1]) + b''.join(parts)


def _chunk(fourcc, payload):
    return fourcc + struct.pack('<I', len(payload)) + payload + (b'\x00' if len(payload) & 1 else b'')


def _u24(v):
    return struct.pack('<I', v)[:3]


def still_file(vp8):
    body = b'WEBP' + _chunk(b'VP8 ', vp8)
    return b'RIFF' + struct.pack('<I', len(body)) + body


def animation_file(streams, width, height, fps=25, loop=0, order=None):
    order = list(range(len(streams))) if order is None else list(order)
    duration = int(math.floor(1000.0 / fps + 0.5))
    body = b'WEBP' + _chunk(b'VP8X', b'\x02\x00\x00\x00' + _u24(width - 1) + _u24(height - 1))
    body += _chunk(b'ANIM', struct.pack('<IH', 0, loop))
    for i in order:
        body += _chunk(b'ANMF', _u24(0) + _u24(0) + _u24(width - 1) + _u24(height - 1) + _u24(duration) + b'\x02' +
                       _chunk(b'VP8 ', streams[i]))
    return b'RIFF' + struct.pack('<I', len(body)) + body


def encode(frames, quality=90):
    """the still .webp file of every frame"""
    return [still_file(encode_frame(f, quality)['vp8']) for f in frames]


def encode_animation(frames, quality=90, fps=25, loop=0, order=None):
    H, W = frames[0].shape[:2]
    return animation_file([encode_frame(f, quality)['vp8'] for f in frames], W, H, fps, loop, order)


# ---- what a decoder shows: the simple loop filter, the chroma upsampling and the colour conversion of libwebp -------------------
def loop_filter(y, level, inner):
    """the format's simple loop filter (sharpness 0) over the luma plane, macroblocks in raster order: the left macroblock edge and
    the three inner vertical edges, then the top edge and the three inner horizontal ones; inner edges only where `inner`"""
    y = y.copy()
    if level == 0:
        return y
    limit = 3 * level

    def edge(p1, p0, q0, q1, thresh):                                 # views of 16 samples each, filtered in place
        a1_, a0_, b0_, b1_ = p1.copy(), p0.copy(), q0.copy(), q1.copy()
        on = 4 * np.abs(a0_ - b0_) + np.abs(a1_ - b1_) <= 2 * thresh + 1
        a = 3 * (b0_ - a0_) + np.clip(a1_ - b1_, -128, 127)
        f1, f2 = np.clip((a + 4) >> 3, -16, 15), np.clip((a + 3) >> 3, -16, 15)
        p0[...] = np.where(on, np.clip(a0_ + f2, 0, 255), a0_)
        q0[...] = np.where(on, np.clip(b0_ - f1, 0, 255), b0_)

    mbh, mbw = inner.shape
    for mby in range(mbh):
        for mbx in range(mbw):
            ys, x0, y0 = slice(16 * mby, 16 * mby + 16), 16 * mbx, 16 * mby
            xs = slice(x0, x0 + 16)
            for k in range(4):
                if (k == 0 and mbx) or (k and inner[mby, mbx]):
                    x = x0 + 4 * k
                    edge(y[ys, x - 2], y[ys, x - 1], y[ys, x], y[ys, x + 1], limit + 4 if k == 0 else limit)
            for k in range(4):
                if (k == 0 and mby) or (k and inner[mby, mbx]):
                    r = y0 + 4 * k
                    edge(y[r - 2, xs], y[r - 1, xs], y[r, xs], y[r + 1, xs], limit + 4 if k == 0 else limit)
    return y


def _upsample(c, H, W):
    """chroma [ceil(H/2), ceil(W/2)] -> [H,W]: (9 near + 3 + 3 + far + 8) >> 4 with replicated edges"""
    c = c[:(H + 1) // 2, :(W + 1) // 2]
    yy, xx = np.arange(H), np.arange(W)
    ny, nx = yy >> 1, xx >> 1
    fy = np.clip(ny + np.where(yy & 1, 1, -1), 0, c.shape[0] - 1)
    fx = np.clip(nx + np.where(xx & 1, 1, -1), 0, c.shape[1] - 1)
    return (9 * c[ny][:, nx] + 3 * c[ny][:, fx] + 3 * c[fy][:, nx] + c[fy][:, fx] + 8) >> 4


def decoded_rgb(result, H, W):
    """the RGB uint8 [H,W,3] that libwebp shows for encode_frame's result"""
    y = loop_filter(result['planes'][0], result['level'], result['inner'])[:H, :W]
    u, v = _upsample(result['planes'][1], H, W), _upsample(result['planes'][2], H, W)
    yy = (y * 19077) >> 8
    r = yy + ((v * 26149) >> 8) - 14234
    g = yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708
    b = yy + ((u * 33050) >> 8) - 17685
    return np.clip(np.stack([r, g, b], axis=2) >> 6, 0, 255).astype(np.uint8)
