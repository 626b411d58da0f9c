"""Decoder package: mirrors `quits.decoder` (/root/reference/src/quits/decoder/__init__.py:3-24)."""
from .base import (detector_error_model_to_matrix, dict_to_csc_matrix_column_row,
                   dict_to_csc_matrix_row_column, spacetime)
from .sliding_window import sliding_window_circuit_mem, sliding_window_phenom_mem
from .bposd import BpOsdDecoder, sliding_window_bposd_circuit_mem, sliding_window_bposd_phenom_mem
from .bplsd import BpLsdDecoder, sliding_window_bplsd_circuit_mem, sliding_window_bplsd_phenom_mem
from .relaybp import RelayBpDecoder, sliding_window_relaybp_circuit_mem, sliding_window_relaybp_phenom_mem
from .whole_history import decode_dem
from .corrections import decode_dem_corrections, sliding_window_corrections
from .soft_outputs import decode_dem_soft_outputs, sliding_window_soft_outputs

__all__ = [
    "dict_to_csc_matrix_column_row",
    "dict_to_csc_matrix_row_column",
    "detector_error_model_to_matrix",
    "spacetime",
    "sliding_window_phenom_mem",
    "sliding_window_circuit_mem",
    "sliding_window_bposd_phenom_mem",
    "sliding_window_bposd_circuit_mem",
    "sliding_window_bplsd_phenom_mem",
    "sliding_window_bplsd_circuit_mem",
    "BpOsdDecoder",
    "BpLsdDecoder",
    "decode_dem",              # beyond the reference's names: any detector error model over its whole history (whole_history.py)
    "sliding_window_corrections",   # ... and the corrections themselves next to the predictions (corrections.py)
    "decode_dem_corrections",
    "sliding_window_soft_outputs",  # ... and a soft record per shot: how sure the decoder was (soft_outputs.py, quits_amd/soft.py)
    "decode_dem_soft_outputs",
    "RelayBpDecoder",          # Relay-BP (relaybp.py, quits_amd/relay.py): a decoder that needs no elimination
    "sliding_window_relaybp_phenom_mem",
    "sliding_window_relaybp_circuit_mem",
]
