"""``from mivos.model.aggregate import aggregate_wbg`` -> the HIP kernel (reference model/aggregate.py:22-37)."""
from eva_vos_amd.stages import aggregate_wbg  # noqa: F401
