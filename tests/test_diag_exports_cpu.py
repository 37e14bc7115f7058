"""The test entry points (zk_diag_*: csrc/diag.hip, and zk_diag_vm_states in csrc/vm_gpu.hip) as the library exports
them.  No GPU: the library loads without one."""
import re
from pathlib import Path

from zkvm_amd import native

ROOT = Path(__file__).resolve().parent.parent

DIAG = [
    "zk_diag_air_fold_host", "zk_diag_air_ws_host", "zk_diag_blake3_host", "zk_diag_blake3_rows",
    "zk_diag_coeff_sources", "zk_diag_column_fills", "zk_diag_composition", "zk_diag_composition_parts",
    "zk_diag_deep", "zk_diag_deep_parts", "zk_diag_detect", "zk_diag_dot_host", "zk_diag_expand_narrow",
    "zk_diag_field_op", "zk_diag_fri_layer", "zk_diag_grind", "zk_diag_hash_rows_virtual", "zk_diag_host_rows",
    "zk_diag_lde", "zk_diag_make_ws_host", "zk_diag_merkle", "zk_diag_mul_limbs_host", "zk_diag_ntt", "zk_diag_ood",
    "zk_diag_row_tasks", "zk_diag_shard_locate", "zk_diag_shard_rounds", "zk_diag_trace_commit", "zk_diag_upload_plan",
    "zk_diag_upload_plan_coeff_src", "zk_diag_vm_states",
]


def test_every_entry_point_resolves():
    assert len(DIAG) == len(set(DIAG)) == 31
    L = native.lib()
    missing = [name for name in DIAG if not hasattr(L, name)]
    assert not missing, missing


def test_every_name_the_python_side_uses_is_listed():
    files = [ROOT / "encrypt-zkvm_amd" / "zkvm_amd" / "native.py"]
    files += sorted((ROOT / "tests").glob("*.py")) + sorted((ROOT / "tools").glob("*.py"))
    used = {}
    for f in files:
        for name in re.findall(r"zk_diag_[a-z0-9_]+", f.read_text()):
            used.setdefault(name, f.name)
    assert len(used) > 20  # (the search found the bindings)
    unknown = {name: where for name, where in used.items() if name not in DIAG}
    assert not unknown, unknown
