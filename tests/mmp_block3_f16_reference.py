"""The float64 model of ``nmpc_mmp_block3_f16``: tests/mmp_block_f16_reference.py on tests/mmp_block3_reference.py."""
import mmp_block3_reference
from mmp_block_f16_reference import Model

_model = Model(mmp_block3_reference)
block, case, emulate, model_chain, rounded = _model.block, _model.case, _model.emulate, _model.model_chain, _model.rounded
