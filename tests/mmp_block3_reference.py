"""The float64 restatement of ``nmpc_mmp_block3_f32`` (the third residual stage, csrc/nmpc_mmp_block3.h), its cases and its derived
bound: the stage LAYER3 of tests/mmp_block_strided_reference.py under the names the tests import."""
from mmp_block_strided_reference import LAYER3

globals().update(LAYER3.names())
