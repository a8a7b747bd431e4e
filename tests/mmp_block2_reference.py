"""The float64 restatement of ``nmpc_mmp_block2_f32`` (the second residual stage, csrc/nmpc_mmp_block2.h), its cases and its derived
bound: the stage LAYER2 of tests/mmp_block_strided_reference.py under the names the tests import."""
from mmp_block_strided_reference import LAYER2

globals().update(LAYER2.names())
