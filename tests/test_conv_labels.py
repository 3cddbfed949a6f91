"""The launch-log label ops.gather_conv_tile answers for a problem, pinned -- no GPU: the planner and the launchers' kernel tables are
host code, and the library loads without a device (tests/test_abi.py).

CASES is a literal record: (n_out, c_in, c_out, in_ld), further arguments of ops.gather_conv_tile, CPD_TUNE knobs -> label. The labels
were recorded on the commit BEFORE the launchers took kernel and label from one table (when the launcher formatted the label next
to a launch ladder and ops.py formatted it once more), so a row that fails says the tables name a kernel differently than the
launcher used to. A new instantiation gets a new row; an existing row changes only when its kernel is renamed on purpose.

Every row of the gather tables that a problem without pointers can reach is here at least once (test_every_reachable_row_is_pinned);
the LDS-epilogue forms (f16e / f16se / f16pe), the unaligned fallbacks and the double-buffered bf16 tile (same label as the
single-buffered one) are what only a launch decides: tests/test_gpu_conv_edges.py reads those from the launch log.
"image" / "plan" stand for the table gather_conv would be given: a dense 3 x 3 table's (frames, h, w), a row plan's rows per tile."""
import types

import pytest

from cpd_amd import ops

KNOBS = ["CPD_GC_ROWWAVE_MIN", "CPD_GC_ROWWAVE_FLOOR", "CPD_GC_ROWWAVE_64", "CPD_GC_ROWWAVE_BN", "CPD_GC_RW8", "CPD_GC_RW8_MIN", "CPD_GC_BF16_MIN",
         "CPD_GC_BF16_MIN64", "CPD_GC_BF16_BN", "CPD_GC_WG", "CPD_GC_BM", "CPD_GC_BN", "CPD_GC_MS", "CPD_GC_NT", "CPD_GC_BF16X3", "CPD_GC_DENSE_ROWWAVE",
         "CPD_GC_BF16_DB", "CPD_GC_PLANNED", "CPD_GC_PLANNED_MIN", "CPD_GC_WINDOW", "CPD_GC_WINDOW_BN", "CPD_GC_WINDOW_SMALL", "CPD_GC_WINDOW_MIN64",
         "CPD_GC_WINDOW_BM256"]

CASES = [
    ((17, 16, 16, 16), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 1}, 'gather_conv_kernel<1,1,true>'),
    ((17, 5, 16, 5), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 1}, 'gather_conv_kernel<1,1,false>'),
    ((17, 16, 32, 16), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 2}, 'gather_conv_kernel<1,2,true>'),
    ((17, 5, 32, 5), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 2}, 'gather_conv_kernel<1,2,false>'),
    ((17, 16, 64, 16), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 4}, 'gather_conv_kernel<1,4,true>'),
    ((17, 5, 64, 5), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 4}, 'gather_conv_kernel<1,4,false>'),
    ((17, 16, 80, 16), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 5}, 'gather_conv_kernel<1,5,true>'),
    ((17, 5, 80, 5), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 5}, 'gather_conv_kernel<1,5,false>'),
    ((17, 16, 128, 16), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 8}, 'gather_conv_kernel<1,8,true>'),
    ((17, 5, 128, 5), {}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 8}, 'gather_conv_kernel<1,8,false>'),
    ((17, 16, 16, 16), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 1}, 'gather_conv_kernel<2,1,true>'),
    ((17, 5, 16, 5), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 1}, 'gather_conv_kernel<2,1,false>'),
    ((17, 16, 32, 16), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 2}, 'gather_conv_kernel<2,2,true>'),
    ((17, 5, 32, 5), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 2}, 'gather_conv_kernel<2,2,false>'),
    ((17, 16, 64, 16), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 4}, 'gather_conv_kernel<2,4,true>'),
    ((17, 5, 64, 5), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 4}, 'gather_conv_kernel<2,4,false>'),
    ((17, 16, 80, 16), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 5}, 'gather_conv_kernel<2,5,true>'),
    ((17, 5, 80, 5), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 5}, 'gather_conv_kernel<2,5,false>'),
    ((17, 16, 128, 16), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 8}, 'gather_conv_kernel<2,8,true>'),
    ((17, 5, 128, 5), {}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 8}, 'gather_conv_kernel<2,8,false>'),
    ((17, 16, 16, 16), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 1}, 'gather_conv_kernel<4,1,true>'),
    ((17, 5, 16, 5), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 1}, 'gather_conv_kernel<4,1,false>'),
    ((17, 16, 32, 16), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 2}, 'gather_conv_kernel<4,2,true>'),
    ((17, 5, 32, 5), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 2}, 'gather_conv_kernel<4,2,false>'),
    ((17, 16, 64, 16), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 4}, 'gather_conv_kernel<4,4,true>'),
    ((17, 5, 64, 5), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 4}, 'gather_conv_kernel<4,4,false>'),
    ((17, 16, 80, 16), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 5}, 'gather_conv_kernel<4,5,true>'),
    ((17, 5, 80, 5), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 5}, 'gather_conv_kernel<4,5,false>'),
    ((17, 16, 128, 16), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 8}, 'gather_conv_kernel<4,8,true>'),
    ((17, 5, 128, 5), {}, {'CPD_GC_MS': 4, 'CPD_GC_NT': 8}, 'gather_conv_kernel<4,8,false>'),
    ((200000, 16, 16, 16), {}, {}, 'gather_conv_kernel<2,1,true>'),
    ((3000, 32, 64, 32), {}, {}, 'gather_conv_kernel<1,1,true>'),
    ((3000, 32, 64, 34), {}, {}, 'gather_conv_kernel<1,1,false>'),
    ((100, 5, 16, 5), {}, {}, 'gather_conv_kernel<1,1,false>'),
    ((33, 16, 16, 16), {'math': 'f16x2', 'in_pairs': True}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 1}, 'gather_conv_h16_kernel<1,1>'),
    ((33, 16, 32, 16), {'math': 'f16x2', 'in_pairs': True}, {'CPD_GC_MS': 1, 'CPD_GC_NT': 2}, 'gather_conv_h16_kernel<1,2>'),
    ((33, 16, 16, 16), {'math': 'f16x2', 'in_pairs': True}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 1}, 'gather_conv_h16_kernel<2,1>'),
    ((33, 16, 32, 16), {'math': 'f16x2', 'in_pairs': True}, {'CPD_GC_MS': 2, 'CPD_GC_NT': 2}, 'gather_conv_h16_kernel<2,2>'),
    ((150000, 16, 32, 16), {'math': 'f16x2', 'in_pairs': True}, {}, 'gather_conv_h16_kernel<2,2>'),
    ((65, 32, 64, 32), {}, {'CPD_GC_WG': 1}, 'tile_conv_kernel<64,64>'),
    ((65, 32, 64, 32), {}, {'CPD_GC_WG': 1, 'CPD_GC_BM': 128}, 'tile_conv_kernel<128,64>'),
    ((65, 32, 128, 32), {}, {'CPD_GC_WG': 1, 'CPD_GC_BN': 128}, 'tile_conv_kernel<64,128>'),
    ((65, 32, 128, 32), {}, {'CPD_GC_WG': 1, 'CPD_GC_BM': 128, 'CPD_GC_BN': 128}, 'tile_conv_kernel<128,128>'),
    ((141376, 256, 256, 256), {'dense': True}, {}, 'tile_conv_kernel<64,128>'),
    ((129, 64, 64, 64), {'dense': True, 'math': 'bf16x3', 'scaled': False}, {'CPD_GC_BF16_MIN': 1}, 'tile_conv_bf16_kernel<128,64>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'bf16x3', 'scaled': False}, {'CPD_GC_BF16_MIN': 1}, 'tile_conv_bf16_kernel<128,128>'),
    ((129, 64, 64, 64), {'dense': True, 'math': 'bf16x3', 'scaled': False}, {'CPD_GC_BF16_MIN': 1000000000, 'CPD_GC_BF16_MIN64': 1}, 'tile_conv_bf16_kernel<64,64>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'bf16x3', 'scaled': False}, {'CPD_GC_BF16_MIN': 1000000000, 'CPD_GC_BF16_MIN64': 1}, 'tile_conv_bf16_kernel<64,128>'),
    ((129, 64, 64, 64), {'dense': True, 'math': 'bf16x3', 'scaled': True}, {'CPD_GC_BF16_MIN': 1}, 'tile_conv_bf16_kernel<128,64>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'bf16x3', 'scaled': True}, {'CPD_GC_BF16_MIN': 1}, 'tile_conv_bf16_kernel<128,128>'),
    ((129, 64, 64, 64), {'dense': True, 'math': 'bf16x3', 'scaled': True}, {'CPD_GC_BF16_MIN': 1000000000, 'CPD_GC_BF16_MIN64': 1}, 'tile_conv_bf16_kernel<64,64>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'bf16x3', 'scaled': True}, {'CPD_GC_BF16_MIN': 1000000000, 'CPD_GC_BF16_MIN64': 1}, 'tile_conv_bf16_kernel<64,128>'),
    ((129, 64, 64, 64), {'dense': True, 'math': 'f16x2', 'scaled': False}, {'CPD_GC_BF16_MIN': 1}, 'tile_conv_f16_kernel<128,64>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'f16x2', 'scaled': False}, {'CPD_GC_BF16_MIN': 1}, 'tile_conv_f16_kernel<128,128>'),
    ((129, 64, 64, 64), {'dense': True, 'math': 'f16x2', 'scaled': False}, {'CPD_GC_BF16_MIN': 1000000000, 'CPD_GC_BF16_MIN64': 1}, 'tile_conv_f16_kernel<64,64>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'f16x2', 'scaled': False}, {'CPD_GC_BF16_MIN': 1000000000, 'CPD_GC_BF16_MIN64': 1}, 'tile_conv_f16_kernel<64,128>'),
    ((129, 64, 64, 64), {'dense': True, 'math': 'f16x2', 'scaled': True}, {'CPD_GC_BF16_MIN': 1}, 'tile_conv_f16s_kernel<128,64>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'f16x2', 'scaled': True}, {'CPD_GC_BF16_MIN': 1}, 'tile_conv_f16s_kernel<128,128>'),
    ((129, 64, 64, 64), {'dense': True, 'math': 'f16x2', 'scaled': True}, {'CPD_GC_BF16_MIN': 1000000000, 'CPD_GC_BF16_MIN64': 1}, 'tile_conv_f16s_kernel<64,64>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'f16x2', 'scaled': True}, {'CPD_GC_BF16_MIN': 1000000000, 'CPD_GC_BF16_MIN64': 1}, 'tile_conv_f16s_kernel<64,128>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'bf16x3'}, {'CPD_GC_BF16_MIN': 1, 'CPD_GC_BF16_DB': 1}, 'tile_conv_bf16_kernel<128,128>'),
    ((129, 64, 128, 64), {'dense': True, 'math': 'f16x2'}, {'CPD_GC_BF16_MIN': 1, 'CPD_GC_BF16_BN': 64}, 'tile_conv_f16_kernel<128,64>'),
    ((141376, 128, 256, 128), {'dense': True, 'math': 'f16x2'}, {}, 'tile_conv_f16_kernel<128,128>'),
    ((35344, 256, 256, 256), {'dense': True, 'math': 'f16x2', 'scaled': True}, {}, 'tile_conv_f16s_kernel<64,128>'),
    ((8000, 27648, 256, 27648), {'dense': True, 'math': 'f16x2', 'scaled': True}, {}, 'tile_conv_f16s_kernel<128,128>'),
    ((35344, 128, 256, 128), {'dense': True, 'bf16x3': True}, {}, 'tile_conv_bf16_kernel<64,128>'),
    ((129, 32, 32, 32), {'math': 'bf16x3', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_bf16_kernel<32,2>'),
    ((129, 64, 64, 64), {'math': 'bf16x3', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_bf16_kernel<64,2>'),
    ((129, 32, 128, 32), {'math': 'bf16x3', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_bf16_kernel<128,2>'),
    ((65, 32, 32, 32), {'math': 'bf16x3', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1000000000, 'CPD_GC_ROWWAVE_FLOOR': 1}, 'rowwave_conv_bf16_kernel<32,1>'),
    ((49, 64, 128, 64), {'math': 'bf16x3', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_bf16_kernel<64,1>'),
    ((65, 32, 128, 32), {'math': 'bf16x3', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_bf16_kernel<128,1>'),
    ((129, 32, 32, 32), {'math': 'f16x2', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16_kernel<32,2>'),
    ((129, 64, 64, 64), {'math': 'f16x2', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16_kernel<64,2>'),
    ((129, 32, 128, 32), {'math': 'f16x2', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16_kernel<128,2>'),
    ((65, 32, 32, 32), {'math': 'f16x2', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1000000000, 'CPD_GC_ROWWAVE_FLOOR': 1}, 'rowwave_conv_f16_kernel<32,1>'),
    ((49, 64, 128, 64), {'math': 'f16x2', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_f16_kernel<64,1>'),
    ((65, 32, 128, 32), {'math': 'f16x2', 'scaled': False, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_f16_kernel<128,1>'),
    ((129, 32, 32, 32), {'math': 'f16x2', 'scaled': True, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16s_kernel<32,2>'),
    ((129, 64, 64, 64), {'math': 'f16x2', 'scaled': True, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16s_kernel<64,2>'),
    ((129, 32, 128, 32), {'math': 'f16x2', 'scaled': True, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16s_kernel<128,2>'),
    ((65, 32, 32, 32), {'math': 'f16x2', 'scaled': True, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 1000000000, 'CPD_GC_ROWWAVE_FLOOR': 1}, 'rowwave_conv_f16s_kernel<32,1>'),
    ((49, 64, 128, 64), {'math': 'f16x2', 'scaled': True, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_f16s_kernel<64,1>'),
    ((65, 32, 128, 32), {'math': 'f16x2', 'scaled': True, 'in_pairs': False}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_f16s_kernel<128,1>'),
    ((129, 32, 32, 32), {'math': 'f16x2', 'scaled': False, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16p_kernel<32,2>'),
    ((129, 64, 64, 64), {'math': 'f16x2', 'scaled': False, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16p_kernel<64,2>'),
    ((129, 32, 128, 32), {'math': 'f16x2', 'scaled': False, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16p_kernel<128,2>'),
    ((65, 32, 32, 32), {'math': 'f16x2', 'scaled': False, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1000000000, 'CPD_GC_ROWWAVE_FLOOR': 1}, 'rowwave_conv_f16p_kernel<32,1>'),
    ((49, 64, 128, 64), {'math': 'f16x2', 'scaled': False, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_f16p_kernel<64,1>'),
    ((65, 32, 128, 32), {'math': 'f16x2', 'scaled': False, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_f16p_kernel<128,1>'),
    ((129, 32, 32, 32), {'math': 'f16x2', 'scaled': True, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16p_kernel<32,2>'),
    ((129, 64, 64, 64), {'math': 'f16x2', 'scaled': True, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16p_kernel<64,2>'),
    ((129, 32, 128, 32), {'math': 'f16x2', 'scaled': True, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1}, 'rowwave_conv_f16p_kernel<128,2>'),
    ((65, 32, 32, 32), {'math': 'f16x2', 'scaled': True, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1000000000, 'CPD_GC_ROWWAVE_FLOOR': 1}, 'rowwave_conv_f16p_kernel<32,1>'),
    ((49, 64, 128, 64), {'math': 'f16x2', 'scaled': True, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_f16p_kernel<64,1>'),
    ((65, 32, 128, 32), {'math': 'f16x2', 'scaled': True, 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 2}, 'rowwave_conv_f16p_kernel<128,1>'),
    ((129, 128, 128, 128), {'math': 'f16x2'}, {'CPD_GC_ROWWAVE_BN': 64}, 'rowwave_conv_f16_kernel<64,2>'),
    ((129, 64, 64, 64), {'math': 'f16x2'}, {'CPD_GC_ROWWAVE_MIN': 2, 'CPD_GC_ROWWAVE_64': 0}, 'rowwave_conv_f16_kernel<64,2>'),
    ((129, 64, 64, 64), {'dense': True, 'math': 'f16x2'}, {'CPD_GC_ROWWAVE_MIN': 1, 'CPD_GC_DENSE_ROWWAVE': 1}, 'rowwave_conv_f16_kernel<64,2>'),
    ((129, 64, 64, 64), {'math': 'f32'}, {'CPD_GC_ROWWAVE_MIN': 1, 'CPD_GC_BF16X3': 2}, 'rowwave_conv_f16_kernel<64,2>'),
    ((400000, 32, 32, 32), {'math': 'f16x2', 'in_pairs': True}, {}, 'rowwave_conv_f16p_kernel<32,2>'),
    ((400000, 32, 32, 32), {'math': 'f16x2', 'scaled': True}, {}, 'rowwave_conv_f16s_kernel<32,2>'),
    ((150000, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True}, {}, 'rowwave_conv_f16p_kernel<64,2>'),
    ((150000, 64, 64, 64), {'math': 'f16x2', 'scaled': True}, {}, 'rowwave_conv_f16s_kernel<64,2>'),
    ((60000, 128, 128, 128), {'math': 'f16x2', 'in_pairs': True}, {}, 'rowwave_conv_f16p_kernel<128,2>'),
    ((60000, 128, 128, 128), {'math': 'f16x2', 'scaled': True}, {}, 'rowwave_conv_f16s_kernel<128,2>'),
    ((20000, 128, 128, 128), {'math': 'f16x2', 'in_pairs': True}, {}, 'rowwave_conv_f16p_kernel<128,1>'),
    ((20000, 128, 128, 128), {'math': 'f16x2', 'scaled': True}, {}, 'rowwave_conv_f16s_kernel<128,1>'),
    ((3000, 128, 128, 128), {'math': 'f16x2', 'in_pairs': True}, {}, 'rowwave_conv_f16p_kernel<32,1>'),
    ((3000, 128, 128, 128), {'math': 'f16x2', 'scaled': True}, {}, 'rowwave_conv_f16s_kernel<32,1>'),
    ((500, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True}, {}, 'rowwave_conv_f16p_kernel<32,1>'),
    ((500, 64, 64, 64), {'math': 'f16x2', 'scaled': True}, {}, 'gather_conv_kernel<1,1,true>'),
    ((257, 32, 32, 32), {'math': 'f16x2', 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1, 'CPD_GC_RW8': 224, 'CPD_GC_RW8_MIN': 1}, 'rowwave_conv_f16pw_kernel<32,8>'),
    ((257, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1, 'CPD_GC_RW8': 224, 'CPD_GC_RW8_MIN': 1}, 'rowwave_conv_f16pw_kernel<64,8>'),
    ((257, 32, 128, 32), {'math': 'f16x2', 'in_pairs': True}, {'CPD_GC_ROWWAVE_MIN': 1, 'CPD_GC_RW8': 224, 'CPD_GC_RW8_MIN': 1}, 'rowwave_conv_f16pw_kernel<128,6>'),
    ((257, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True, 'scaled': True}, {'CPD_GC_ROWWAVE_MIN': 1, 'CPD_GC_RW8': 224, 'CPD_GC_RW8_MIN': 1}, 'rowwave_conv_f16pw_kernel<64,8>'),
    ((257, 64, 64, 64), {'math': 'f16x2'}, {'CPD_GC_ROWWAVE_MIN': 1, 'CPD_GC_RW8': 224, 'CPD_GC_RW8_MIN': 1}, 'rowwave_conv_f16_kernel<64,2>'),
    ((100000, 64, 64, 64), {'math': 'f16x2', 'kv': 27}, {}, 'rowwave_conv_f16_kernel<64,2>'),
    ((100000, 64, 64, 64), {'math': 'f16x2', 'kv': 28}, {}, 'rowwave_conv_f16_kernel<64,2>'),
    ((100000, 64, 64, 64), {'math': 'f16x2', 'kv': 29}, {}, 'tile_conv_f16_kernel<128,64>'),
    ((100000, 64, 64, 64), {'math': 'f16x2', 'kv': 125}, {}, 'tile_conv_f16_kernel<128,64>'),
    ((100000, 64, 64, 64), {'math': 'f16x2', 'kv': 125, 'scaled': True}, {}, 'tile_conv_f16s_kernel<128,64>'),
    ((100000, 64, 64, 64), {'math': 'bf16x3', 'kv': 125}, {}, 'tile_conv_bf16_kernel<128,64>'),
    ((3000, 32, 32, 32), {'math': 'f16x2', 'kv': 125}, {}, 'gather_conv_kernel<1,1,true>'),
    ((3000, 32, 32, 32), {'math': 'f16x2', 'kv': 125, 'in_pairs': True}, {}, 'gather_conv_kernel<1,1,true>'),
    ((257, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True, 'kv': 125}, {'CPD_GC_ROWWAVE_MIN': 1, 'CPD_GC_RW8': 224, 'CPD_GC_RW8_MIN': 1}, 'gather_conv_kernel<1,1,true>'),
    ((129, 64, 128, 64), {'math': 'f16x2', 'kv': 125, 'scaled': True}, {'CPD_GC_ROWWAVE_MIN': 1, 'CPD_GC_BF16_MIN': 1}, 'tile_conv_f16s_kernel<128,128>'),
    ((141376, 128, 128, 128), {'math': 'f16x2', 'dense': True, 'image': (4, 188, 188)}, {}, 'window_conv_f16_kernel<128>'),
    ((141376, 128, 128, 128), {'math': 'f16x2', 'scaled': True, 'dense': True, 'image': (4, 188, 188)}, {}, 'window_conv_f16s_kernel<128>'),
    ((141376, 128, 128, 128), {'bf16x3': True, 'dense': True, 'image': (4, 188, 188)}, {}, 'window_conv_bf16_kernel<128>'),
    ((1131008, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True, 'dense': True, 'image': (8, 376, 376)}, {}, 'window_conv_f16_kernel<64,256>'),
    ((1131008, 64, 64, 64), {'math': 'f16x2', 'scaled': True, 'dense': True, 'image': (8, 376, 376)}, {}, 'window_conv_f16s_kernel<64,256>'),
    ((1131008, 64, 11, 64), {'math': 'f16x2', 'dense': True, 'image': (8, 376, 376)}, {}, 'window_conv_f16_kernel<16,256>'),
    ((35344, 128, 128, 128), {'math': 'f16x2', 'dense': True, 'image': (1, 188, 188)}, {}, 'window_conv_f16_kernel<64>'),
    ((8836, 256, 256, 256), {'math': 'f16x2', 'dense': True, 'image': (1, 94, 94)}, {}, 'tile_conv_f16_kernel<64,128>'),
    ((400, 64, 64, 64), {'math': 'f16x2', 'scaled': True, 'dense': True, 'image': (1, 20, 20)}, {}, 'gather_conv_kernel<1,1,true>'),
    ((141376, 128, 128, 128), {'math': 'f32', 'dense': True, 'image': (4, 188, 188)}, {}, 'tile_conv_kernel<64,128>'),
    ((35344, 128, 128, 130), {'math': 'f16x2', 'dense': True, 'image': (1, 188, 188)}, {}, 'gather_conv_kernel<2,2,false>'),
    ((100000, 32, 32, 32), {'math': 'f16x2', 'in_pairs': True, 'plan': 128}, {}, 'rowplan_conv_f16p_kernel<32>'),
    ((100000, 128, 128, 128), {'math': 'f16x2', 'in_pairs': True, 'plan': 128}, {}, 'rowplan_conv_f16p_kernel<128>'),
    ((1000, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True, 'plan': 128}, {}, 'rowwave_conv_f16p_kernel<32,1>'),
    ((100000, 32, 32, 32), {'math': 'f16x2', 'in_pairs': True, 'plan': 256}, {}, 'rowplan_conv_f16p_kernel<32,256>'),
    ((100000, 128, 128, 128), {'math': 'f16x2', 'in_pairs': True, 'plan': 256}, {}, 'rowplan_conv_f16p_kernel<128,256>'),
    ((1000, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True, 'plan': 256}, {}, 'rowwave_conv_f16p_kernel<32,1>'),
    ((100000, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True, 'plan': 128, 'scaled': True}, {}, 'rowwave_conv_f16p_kernel<64,2>'),
    ((1000, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True, 'plan': 256}, {'CPD_GC_PLANNED_MIN': 1}, 'rowplan_conv_f16p_kernel<64,256>'),
    ((100000, 64, 64, 64), {'math': 'f16x2', 'in_pairs': True, 'plan': 128}, {'CPD_GC_PLANNED': 0}, 'rowwave_conv_f16p_kernel<64,2>'),
]


def told(case, mp):
    (n_out, c_in, c_out, in_ld), kw, knobs, _ = case
    mp.setenv("CPD_TUNE", "1")                   # the knobs are only read when this is set
    for k in KNOBS:
        mp.delenv(k, raising=False)
    for k, v in knobs.items():
        assert k in KNOBS, k
        mp.setenv(k, str(v))
    kw = dict(kw)
    image, plan = kw.pop("image", None), kw.pop("plan", None)
    if image or plan:
        kw["nbr"] = types.SimpleNamespace(image=image, plan=(None, None, None, plan) if plan else None, shape=(9 if image else 27, n_out))
    return ops.gather_conv_tile(n_out, c_in, c_out, in_ld, **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d" % (c[3], CASES.index(c)))
def test_label_is_the_recorded_one(case, monkeypatch):
    assert told(case, monkeypatch) == case[3]


def test_every_reachable_row_is_pinned():
    """the families of the gather tables, spelled out independently of the record: each label appears in CASES"""
    want = {"gather_conv_kernel<%d,%d,%s>" % (ms, nt, v) for ms in (1, 2, 4) for nt in (1, 2, 4, 5, 8) for v in ("true", "false")}
    want |= {"gather_conv_h16_kernel<%d,%d>" % (ms, nt) for ms in (1, 2) for nt in (1, 2)}
    want |= {"tile_conv_%skernel<%d,%d>" % (f, bm, bn) for f in ("", "bf16_", "f16_", "f16s_") for bm in (64, 128) for bn in (64, 128)}
    want |= {"rowwave_conv_%s_kernel<%d,%d>" % (f, bn, ms) for f in ("bf16", "f16", "f16s", "f16p") for bn in (32, 64, 128) for ms in (1, 2)}
    want |= {"rowwave_conv_f16pw_kernel<32,8>", "rowwave_conv_f16pw_kernel<64,8>", "rowwave_conv_f16pw_kernel<128,6>"}
    assert want <= {c[3] for c in CASES}, sorted(want - {c[3] for c in CASES})


def test_the_replan_and_the_scaled_forms_are_pinned():
    """the issue's two special cases: 125 taps are planned as a dense layer, and an absmax block selects the f16s forms"""
    assert any(c[1].get("kv") == 125 and c[3].startswith("tile_conv_") for c in CASES)
    assert any(c[1].get("kv") == 27 and c[3].startswith("rowwave_conv_") for c in CASES)
    assert any(c[1].get("scaled") and "_f16s_kernel" in c[3] for c in CASES)
