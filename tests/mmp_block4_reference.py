"""The float64 restatement of ``nmpc_mmp_block4_f32`` (the fourth residual stage, csrc/nmpc_mmp_block4.h), its cases and its derived
bound: the stage LAYER4 of tests/mmp_block_strided_reference.py under the names the tests import."""
from mmp_block_strided_reference import LAYER4

globals().update(LAYER4.names())
