"""ctypes binding of ``librcdc.so`` (the C ABI declared in ``include/rcdc.h``).

The library is built in-tree by ``__graft_entry__.build()`` /
``rustic_core_amd/csrc/Makefile``.  There is no fallback: if the shared
library is missing or a symbol is absent, loading raises ``RcdcLibraryError``
-- the chunker never silently runs on the CPU.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librcdc.so")
# A/B builds of the same sources (tools/ab_lib.sh) load from RCDC_LIB instead
if os.environ.get("RCDC_LIB"):
    LIB_PATH = os.path.abspath(os.environ["RCDC_LIB"])
CSRC = os.path.join(_HERE, "csrc")

# Every entry point of include/rcdc.h (checked by tests/test_abi.py).
EXPORTS = (
    "rcdc_abi_version", "rcdc_last_error", "rcdc_check_params", "rcdc_parse_poly",
    "rcdc_ctx_create", "rcdc_ctx_destroy", "rcdc_max_cuts", "rcdc_chunk_batch",
    "rcdc_stream_open", "rcdc_stream_feed", "rcdc_stream_close", "rcdc_plan_create",
    "rcdc_plan_destroy", "rcdc_plan_run", "rcdc_plan_results", "rcdc_plan_device_results",
    "rcdc_plan_get_info", "rcdc_plan_set_timing", "rcdc_plan_kernel_times", "rcdc_fixed_cuts",
    "rcdc_sha256_chunks", "rcdc_plan_hash", "rcdc_plan_digests", "rcdc_plan_device_digests",
    "rcdc_plan_set_pipeline", "rcdc_plan_hash_many", "rcdc_plan_walk_stats",
    "rcdc_plan_finish", "rcdc_stream_queued", "rcdc_stream_batch_bytes",
    "rcdc_aead_seal", "rcdc_aead_open", "rcdc_pack_build",
    "rcdc_zstd_bound", "rcdc_zstd_compress", "rcdc_zstd_tables", "rcdc_zstd_tables_size",
    "rcdc_zstd_check", "rcdc_pack_build_raw", "rcdc_pack_build_raw_multi", "rcdc_copy_ranges",
    "rcdc_sha256_host", "rcdc_host_alloc", "rcdc_host_free", "rcdc_plan_window",
    "rcdc_ingest_config_default", "rcdc_ingest_create", "rcdc_ingest_add_index",
    "rcdc_ingest_reserve", "rcdc_ingest_commit", "rcdc_ingest_add", "rcdc_ingest_flush",
    "rcdc_ingest_finish", "rcdc_ingest_destroy", "rcdc_sha256_host_one",
    "rcdc_sha256_host_ni", "rcdc_ingest_cancel", "rcdc_ingest_stream_open",
    "rcdc_ingest_stream_reserve", "rcdc_ingest_stream_close", "rcdc_ingest_stream_abort",
    "rcdc_ingest_footprint", "rcdc_ingest_mem_live", "rcdc_index_create", "rcdc_index_destroy",
    "rcdc_index_add", "rcdc_index_size", "rcdc_ingest_set_index",
    "rcdc_zstd_decompress", "rcdc_zstd_frame_info", "rcdc_zstd_decompress_stats",
    "rcdc_place_blobs",
    "rcdc_dindex_create", "rcdc_dindex_destroy", "rcdc_dindex_size", "rcdc_dindex_keys",
    "rcdc_dindex_add", "rcdc_dindex_lookup", "rcdc_dindex_first_new",
    "rcdc_index_parse", "rcdc_index_parse_bound", "rcdc_index_parse_tile",
    "rcdc_prune_create", "rcdc_prune_destroy", "rcdc_prune_set_entries", "rcdc_prune_mark",
    "rcdc_prune_keep",
    "rcdc_index_write", "rcdc_index_write_bound", "rcdc_index_write_span",
    "rcdc_tree_parse", "rcdc_tree_parse_bound", "rcdc_tree_parse_tile",
    "rcdc_tree_nodes", "rcdc_tree_nodes_bound", "rcdc_tree_names", "rcdc_check_trees_level",
    "rcdc_pack_header_parse", "rcdc_pack_header_parse_bound", "rcdc_pack_header_parse_tile",
    "rcdc_check_packs", "rcdc_check_packs_sort_max",
    "rcdc_repair_trees_level", "rcdc_repair_spread", "rcdc_repair_spread_rounds_per_launch",
)
ABI_VERSION = 5


class RcdcLibraryError(RuntimeError):
    """librcdc.so could not be loaded (not built, wrong ABI)."""


class Buf(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_uint64)]


class PlanInfo(ctypes.Structure):
    _fields_ = [
        ("scanned_bytes", ctypes.c_uint64),
        ("segments", ctypes.c_uint64),
        ("segment_bytes", ctypes.c_uint32),
        ("work_items", ctypes.c_uint32),
        ("scan_blocks", ctypes.c_uint32),
        ("walk_pieces", ctypes.c_uint32),
        ("walk_seg_bytes", ctypes.c_uint32),
        ("pad", ctypes.c_uint32),
    ]


class DindexLoc(ctypes.Structure):
    """rcdc_dindex_loc."""
    _fields_ = [("pack", ctypes.c_uint32), ("offset", ctypes.c_uint32),
                ("length", ctypes.c_uint32), ("uncompressed_length", ctypes.c_uint32)]


class DindexHit(ctypes.Structure):
    """rcdc_dindex_hit."""
    _fields_ = [("entry", ctypes.c_uint32), ("count", ctypes.c_uint32), ("loc", DindexLoc)]


class IxparseRef(ctypes.Structure):
    """rcdc_ixparse_ref."""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64)]


class IxparseFile(ctypes.Structure):
    """rcdc_ixparse_file."""
    _fields_ = [("status", ctypes.c_uint32), ("packs", ctypes.c_uint32 * 2),
                ("packs_to_delete", ctypes.c_uint32), ("entries", ctypes.c_uint32 * 2)]


class IxparsePack(ctypes.Structure):
    """rcdc_ixparse_pack."""
    _fields_ = [("id", ctypes.c_uint8 * 32), ("type", ctypes.c_uint32),
                ("number", ctypes.c_uint32), ("size", ctypes.c_uint64)]


class IxparseResult(ctypes.Structure):
    """rcdc_ixparse_result."""
    _fields_ = [("packs", ctypes.c_uint64 * 2), ("entries", ctypes.c_uint64 * 2),
                ("files_not_parsed", ctypes.c_uint64)]


class IxwritePack(ctypes.Structure):
    """rcdc_ixwrite_pack."""
    _fields_ = [("id", ctypes.c_uint8 * 32), ("first", ctypes.c_uint64),
                ("count", ctypes.c_uint32), ("type", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("size", ctypes.c_uint32),
                ("time_off", ctypes.c_uint32), ("time_len", ctypes.c_uint32)]


class IxwriteFile(ctypes.Structure):
    """rcdc_ixwrite_file."""
    _fields_ = [("pack_first", ctypes.c_uint64), ("pack_count", ctypes.c_uint32),
                ("n_delete", ctypes.c_uint32), ("sup_first", ctypes.c_uint64),
                ("sup_count", ctypes.c_uint32), ("has_supersedes", ctypes.c_uint32)]


class IxwriteOut(ctypes.Structure):
    """rcdc_ixwrite_out."""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64)]


class TrparseResult(ctypes.Structure):
    """rcdc_trparse_result."""
    _fields_ = [("data_ids", ctypes.c_uint64), ("tree_ids", ctypes.c_uint64),
                ("nodes", ctypes.c_uint64), ("blobs_not_parsed", ctypes.c_uint64)]


class PkhdrResult(ctypes.Structure):
    """rcdc_pkhdr_result."""
    _fields_ = [("packs", ctypes.c_uint64 * 2), ("entries", ctypes.c_uint64 * 2),
                ("headers_not_parsed", ctypes.c_uint64)]


class CkpackResult(ctypes.Structure):
    """rcdc_ckpack_result."""
    _fields_ = [("findings", ctypes.c_uint64), ("packs_host", ctypes.c_uint64),
                ("packs_sorted_on_device", ctypes.c_uint64)]


class RepairLevelResult(ctypes.Structure):
    """rcdc_repair_level_result."""
    _fields_ = [("missing_ids", ctypes.c_uint64), ("damaged_nodes", ctypes.c_uint64),
                ("files_without_content", ctypes.c_uint64),
                ("first_without_content", ctypes.c_uint64)]


class PruneResult(ctypes.Structure):
    """rcdc_prune_result."""
    _fields_ = [("missing", ctypes.c_uint64), ("first_missing", ctypes.c_uint64),
                ("dup_entries", ctypes.c_uint64), ("rounds", ctypes.c_uint32),
                ("pad", ctypes.c_uint32), ("mark_ms", ctypes.c_float),
                ("sums_ms", ctypes.c_float)]


def build(verbose: bool = False) -> str:
    """Compile librcdc.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-s", "-j8", "-C", CSRC], capture_output=not verbose, text=True)
    if out.returncode != 0:
        raise RcdcLibraryError(f"building librcdc.so failed:\n{out.stdout}\n{out.stderr}")
    return LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch ships its own libamdhip64 (soname
    # libamdhip64.so.7, but NEEDED as "libamdhip64.so").  Loading torch first
    # makes librcdc bind to that already-loaded runtime; loading librcdc
    # first would pull /opt/rocm's copy and torch would then load a second
    # one ("no ROCm-capable device" from whichever initialises last).
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover - torch-free embedding
        pass
    if not os.path.exists(LIB_PATH):
        raise RcdcLibraryError(
            f"{LIB_PATH} not found: build it with __graft_entry__.build() "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - environment specific
        raise RcdcLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name in EXPORTS:
        if not hasattr(L, name):
            raise RcdcLibraryError(f"{LIB_PATH} lacks symbol {name}")
    u64, u32, vp, st = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int
    P = ctypes.POINTER
    L.rcdc_abi_version.restype = u32
    L.rcdc_abi_version.argtypes = []
    if L.rcdc_abi_version() != ABI_VERSION:
        raise RcdcLibraryError("librcdc.so ABI version mismatch")
    L.rcdc_last_error.restype = ctypes.c_char_p
    L.rcdc_last_error.argtypes = []
    L.rcdc_check_params.restype = st
    L.rcdc_check_params.argtypes = [u64, u64, u64]
    L.rcdc_parse_poly.restype = st
    L.rcdc_parse_poly.argtypes = [ctypes.c_char_p, P(u64)]
    L.rcdc_ctx_create.restype = st
    L.rcdc_ctx_create.argtypes = [u64, u64, u64, u64, ctypes.c_int, P(vp)]
    L.rcdc_ctx_destroy.restype = None
    L.rcdc_ctx_destroy.argtypes = [vp]
    L.rcdc_max_cuts.restype = u64
    L.rcdc_max_cuts.argtypes = [vp, u64]
    L.rcdc_chunk_batch.restype = st
    L.rcdc_chunk_batch.argtypes = [vp, P(Buf), u32, vp, u64, vp]
    L.rcdc_stream_open.restype = st
    L.rcdc_stream_open.argtypes = [vp, P(vp)]
    L.rcdc_stream_feed.restype = st
    L.rcdc_stream_feed.argtypes = [vp, vp, u64, ctypes.c_int, vp, u64, P(u64)]
    L.rcdc_stream_queued.restype = u64
    L.rcdc_stream_queued.argtypes = [vp]
    L.rcdc_stream_batch_bytes.restype = u64
    L.rcdc_stream_batch_bytes.argtypes = [vp]
    L.rcdc_plan_finish.restype = st
    L.rcdc_plan_finish.argtypes = [vp]
    L.rcdc_stream_close.restype = None
    L.rcdc_stream_close.argtypes = [vp]
    L.rcdc_plan_create.restype = st
    L.rcdc_plan_create.argtypes = [vp, vp, vp, u32, u64, P(vp)]
    L.rcdc_plan_destroy.restype = None
    L.rcdc_plan_destroy.argtypes = [vp]
    L.rcdc_plan_run.restype = st
    L.rcdc_plan_run.argtypes = [vp, vp, vp]
    L.rcdc_plan_results.restype = st
    L.rcdc_plan_results.argtypes = [vp, vp, u64, vp]
    L.rcdc_plan_device_results.restype = st
    L.rcdc_plan_device_results.argtypes = [vp, P(u64), P(u64), P(P(u64))]
    L.rcdc_plan_get_info.restype = st
    L.rcdc_plan_get_info.argtypes = [vp, P(PlanInfo)]
    L.rcdc_plan_set_timing.restype = st
    L.rcdc_plan_set_timing.argtypes = [vp, ctypes.c_int]
    L.rcdc_plan_kernel_times.restype = st
    L.rcdc_plan_kernel_times.argtypes = [vp, P(u64), P(ctypes.c_double), P(ctypes.c_double)]
    L.rcdc_fixed_cuts.restype = u64
    L.rcdc_fixed_cuts.argtypes = [u64, u64, vp, u64]
    L.rcdc_sha256_chunks.restype = st
    L.rcdc_sha256_chunks.argtypes = [vp, vp, vp, u32, vp, vp]
    L.rcdc_plan_hash.restype = st
    L.rcdc_plan_hash.argtypes = [vp, vp, vp]
    L.rcdc_plan_digests.restype = st
    L.rcdc_plan_digests.argtypes = [vp, vp, u64, vp]
    L.rcdc_plan_hash_many.restype = st
    L.rcdc_plan_hash_many.argtypes = [vp, u32, vp, vp]
    L.rcdc_plan_set_pipeline.restype = st
    L.rcdc_plan_set_pipeline.argtypes = [vp, ctypes.c_int]
    L.rcdc_plan_walk_stats.restype = st
    L.rcdc_plan_walk_stats.argtypes = [vp, vp, vp, u64]
    L.rcdc_aead_seal.restype = st
    L.rcdc_aead_seal.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    L.rcdc_aead_open.restype = st
    L.rcdc_aead_open.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp]
    L.rcdc_pack_build.restype = st
    L.rcdc_pack_build.argtypes = [vp, vp, vp, vp, u32, vp, u32, vp, u64, vp, vp]
    L.rcdc_pack_build_raw.restype = st
    L.rcdc_pack_build_raw.argtypes = [vp, vp, vp, vp, u32, vp, u32, vp, u64, vp, vp]
    L.rcdc_pack_build_raw_multi.restype = st
    L.rcdc_pack_build_raw_multi.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, vp, u64, vp, vp]
    L.rcdc_copy_ranges.restype = st
    L.rcdc_copy_ranges.argtypes = [vp, vp, u32, vp, u32, vp, vp]
    L.rcdc_place_blobs.restype = st
    L.rcdc_place_blobs.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, u32, u32, vp, vp]
    L.rcdc_sha256_host.restype = st
    L.rcdc_sha256_host.argtypes = [vp, vp, u32, vp]
    L.rcdc_host_alloc.restype = st
    L.rcdc_host_alloc.argtypes = [u64, vp]
    L.rcdc_host_free.restype = None
    L.rcdc_host_free.argtypes = [vp]
    L.rcdc_zstd_bound.restype = u64
    L.rcdc_zstd_bound.argtypes = [u64]
    L.rcdc_zstd_compress.restype = st
    L.rcdc_zstd_compress.argtypes = [vp, ctypes.c_int, vp, vp, u32, vp, vp, vp]
    L.rcdc_zstd_check.restype = st
    L.rcdc_zstd_check.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp]
    L.rcdc_zstd_decompress.restype = st
    L.rcdc_zstd_decompress.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp]
    L.rcdc_zstd_frame_info.restype = st
    L.rcdc_zstd_frame_info.argtypes = [vp, u64, P(u64), P(u64), P(u32)]
    L.rcdc_zstd_decompress_stats.restype = st
    L.rcdc_zstd_decompress_stats.argtypes = [vp, vp]
    L.rcdc_zstd_tables.restype = None
    L.rcdc_zstd_tables.argtypes = [vp]
    L.rcdc_zstd_tables_size.restype = u64
    L.rcdc_zstd_tables_size.argtypes = []
    L.rcdc_ingest_config_default.restype = None
    L.rcdc_ingest_config_default.argtypes = [vp]
    L.rcdc_ingest_create.restype = st
    L.rcdc_ingest_create.argtypes = [vp, vp, vp, vp, vp, P(vp)]
    L.rcdc_ingest_add_index.restype = st
    L.rcdc_ingest_add_index.argtypes = [vp, vp, u64]
    L.rcdc_ingest_reserve.restype = st
    L.rcdc_ingest_reserve.argtypes = [vp, u64, P(vp), P(u64)]
    L.rcdc_ingest_commit.restype = st
    L.rcdc_ingest_commit.argtypes = [vp, u64, u64, u64]
    L.rcdc_ingest_add.restype = st
    L.rcdc_ingest_add.argtypes = [vp, u64, vp, u64]
    L.rcdc_ingest_flush.restype = st
    L.rcdc_ingest_flush.argtypes = [vp]
    L.rcdc_ingest_finish.restype = st
    L.rcdc_ingest_finish.argtypes = [vp, vp]
    L.rcdc_ingest_destroy.restype = None
    L.rcdc_ingest_destroy.argtypes = [vp]
    L.rcdc_sha256_host_one.restype = st
    L.rcdc_sha256_host_one.argtypes = [vp, u64, vp]
    L.rcdc_sha256_host_ni.restype = st
    L.rcdc_sha256_host_ni.argtypes = [vp, vp, u32, u32, vp]
    L.rcdc_ingest_cancel.restype = st
    L.rcdc_ingest_cancel.argtypes = [vp, u64]
    L.rcdc_ingest_stream_open.restype = st
    L.rcdc_ingest_stream_open.argtypes = [vp, u64, u64, P(u64)]
    L.rcdc_ingest_stream_reserve.restype = st
    L.rcdc_ingest_stream_reserve.argtypes = [vp, u64, u64, P(vp), P(u64)]
    L.rcdc_ingest_stream_close.restype = st
    L.rcdc_ingest_stream_close.argtypes = [vp, u64]
    L.rcdc_ingest_stream_abort.restype = st
    L.rcdc_ingest_stream_abort.argtypes = [vp, u64]
    L.rcdc_ingest_footprint.restype = st
    L.rcdc_ingest_footprint.argtypes = [vp, vp, P(u64), P(u64)]
    L.rcdc_ingest_mem_live.restype = None
    L.rcdc_ingest_mem_live.argtypes = [P(u64), P(u64)]
    L.rcdc_index_create.restype = st
    L.rcdc_index_create.argtypes = [P(vp)]
    L.rcdc_index_destroy.restype = None
    L.rcdc_index_destroy.argtypes = [vp]
    L.rcdc_index_add.restype = st
    L.rcdc_index_add.argtypes = [vp, vp, u64]
    L.rcdc_index_size.restype = u64
    L.rcdc_index_size.argtypes = [vp]
    L.rcdc_ingest_set_index.restype = st
    L.rcdc_ingest_set_index.argtypes = [vp, vp]
    L.rcdc_plan_window.restype = st
    L.rcdc_plan_window.argtypes = [vp, u32, u64, u32, vp, vp]
    L.rcdc_plan_device_digests.restype = st
    L.rcdc_plan_device_digests.argtypes = [vp, P(u64)]
    L.rcdc_dindex_create.restype = st
    L.rcdc_dindex_create.argtypes = [vp, u64, P(vp)]
    L.rcdc_dindex_destroy.restype = None
    L.rcdc_dindex_destroy.argtypes = [vp]
    L.rcdc_dindex_size.restype = u64
    L.rcdc_dindex_size.argtypes = [vp]
    L.rcdc_dindex_keys.restype = u64
    L.rcdc_dindex_keys.argtypes = [vp]
    L.rcdc_dindex_add.restype = st
    L.rcdc_dindex_add.argtypes = [vp, vp, vp, u64, u32, vp]
    L.rcdc_dindex_lookup.restype = st
    L.rcdc_dindex_lookup.argtypes = [vp, vp, u64, vp, vp]
    L.rcdc_dindex_first_new.restype = st
    L.rcdc_dindex_first_new.argtypes = [vp, vp, u64, vp, vp, vp]
    L.rcdc_index_parse_bound.restype = None
    L.rcdc_index_parse_bound.argtypes = [u64, P(u64), P(u64)]
    L.rcdc_index_parse_tile.restype = u32
    L.rcdc_index_parse_tile.argtypes = []
    L.rcdc_index_parse.restype = st
    L.rcdc_index_parse.argtypes = [vp, vp, u64, vp, u32, vp, vp, vp, u64, vp, vp, u64, vp, vp]
    L.rcdc_prune_create.restype = st
    L.rcdc_prune_create.argtypes = [vp, vp, u64, vp, P(vp)]
    L.rcdc_prune_destroy.restype = None
    L.rcdc_prune_destroy.argtypes = [vp]
    L.rcdc_prune_set_entries.restype = st
    L.rcdc_prune_set_entries.argtypes = [vp, vp, u64, vp, u64, vp, u64, u64, vp, u64, vp]
    L.rcdc_prune_mark.restype = st
    L.rcdc_prune_mark.argtypes = [vp, vp, vp, vp, P(PruneResult), vp]
    L.rcdc_prune_keep.restype = st
    L.rcdc_prune_keep.argtypes = [vp, vp, vp, vp, vp]
    L.rcdc_index_write_bound.restype = u64
    L.rcdc_index_write_bound.argtypes = [u64, u64, u64, u64, u64]
    L.rcdc_index_write_span.restype = u32
    L.rcdc_index_write_span.argtypes = []
    L.rcdc_index_write.restype = st
    L.rcdc_index_write.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, u64, vp, u64, vp, u32,
                                   vp, u64, vp, u64, vp, u64, vp, P(u64), vp]
    L.rcdc_tree_parse_bound.restype = None
    L.rcdc_tree_parse_bound.argtypes = [u64, P(u64), P(u64), P(u64)]
    L.rcdc_tree_parse_tile.restype = u32
    L.rcdc_tree_parse_tile.argtypes = []
    L.rcdc_tree_parse.restype = st
    L.rcdc_tree_parse.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp, vp, u64, vp, vp, vp]
    L.rcdc_tree_nodes_bound.restype = None
    L.rcdc_tree_nodes_bound.argtypes = [u64, P(u64), P(u64), P(u64)]
    L.rcdc_tree_nodes.restype = st
    L.rcdc_tree_nodes.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp, vp, u64, vp, u64, vp, vp, vp]
    L.rcdc_tree_names.restype = st
    L.rcdc_tree_names.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, vp, u64, P(u64), vp]
    L.rcdc_check_trees_level.restype = st
    L.rcdc_check_trees_level.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, u64, vp, u64, vp,
                                         u64, vp, u64, P(u64), vp]
    L.rcdc_pack_header_parse_bound.restype = u64
    L.rcdc_pack_header_parse_bound.argtypes = [u64]
    L.rcdc_pack_header_parse_tile.restype = u32
    L.rcdc_pack_header_parse_tile.argtypes = []
    L.rcdc_pack_header_parse.restype = st
    L.rcdc_pack_header_parse.argtypes = [vp, vp, u64, vp, u32, vp, vp, vp, u64, vp, vp, vp]
    L.rcdc_check_packs_sort_max.restype = u32
    L.rcdc_check_packs_sort_max.argtypes = []
    L.rcdc_check_packs.restype = st
    L.rcdc_check_packs.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64,
                                   vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]
    L.rcdc_repair_trees_level.restype = st
    L.rcdc_repair_trees_level.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, u64, vp, u64, vp,
                                          P(RepairLevelResult), vp]
    L.rcdc_repair_spread.restype = st
    L.rcdc_repair_spread.argtypes = [vp, vp, u64, vp, vp, u64, P(u64), vp]
    L.rcdc_repair_spread_rounds_per_launch.restype = u32
    L.rcdc_repair_spread_rounds_per_launch.argtypes = []
    _lib = L
    return L


def last_error() -> str:
    return lib().rcdc_last_error().decode(errors="replace")
