"""rustic_core_amd -- MI355X-native content-defined chunker for rustic_core.

Replaces the Rabin CDC hot path of rustic_core (crates/core/src/chunker*)
with hand-written gfx950 HIP kernels behind the C ABI of ``include/rcdc.h``
(``librcdc.so``).  The Python layer mirrors the reference's chunker surface
(``ChunkIter.from_config``, ``check_rabin_params``, ``ConfigFile``) and the
device-resident batch API used by ``bench.py``.
"""
from .errors import ErrorKind, RusticError  # noqa: F401
from .chunker import (  # noqa: F401
    Chunker, ChunkIter, ConfigFile, Context, RabinChunkIter, FixedSizeChunkIter,
    check_rabin_params, fixed_cuts, DEFAULT_CHUNK_SIZE, DEFAULT_CHUNK_MIN_SIZE,
    DEFAULT_CHUNK_MAX_SIZE,
)
from .restore import RestorePlan, index_lookup, restore_contents  # noqa: F401
from .dindex import DeviceIndex, IndexType  # noqa: F401
from .repack import (  # noqa: F401
    BlobCopier, CopyPackBlobs, CopyStats, NewPack, plan_copy, plan_repack,
)
from .prune import (  # noqa: F401
    LimitOption, PackStatus, PackToDo, PrunePlan, PruneOptions, PruneStats,
)
from .index_write import (  # noqa: F401
    DeviceIndexer, FileRecord, PackRecord, WrittenJson, save_index_files, write_json,
)
from .tree import (  # noqa: F401
    ParsedTrees, find_used_blobs, parse_tree_host, parse_trees, snapshot_trees,
)
from .headers import (  # noqa: F401
    HeaderResult, PackChecker, ParsedHeaders, RepairReport, index_checked, parse_headers,
    read_headers, repair_index,
)
from .repair import (  # noqa: F401
    RepairPlan, RepairResult, RepairSnapshotsOptions, apply_repair, plan_repair, repair_snapshots,
)

__all__ = [
    "ErrorKind", "RusticError", "Chunker", "ChunkIter", "ConfigFile", "Context",
    "RabinChunkIter", "FixedSizeChunkIter", "check_rabin_params", "fixed_cuts",
    "RestorePlan", "index_lookup", "restore_contents", "DeviceIndex", "IndexType",
    "BlobCopier", "CopyPackBlobs", "CopyStats", "NewPack", "plan_copy", "plan_repack",
    "LimitOption", "PackStatus", "PackToDo", "PrunePlan", "PruneOptions", "PruneStats",
    "DeviceIndexer", "FileRecord", "PackRecord", "WrittenJson", "save_index_files", "write_json",
    "ParsedTrees", "find_used_blobs", "parse_tree_host", "parse_trees", "snapshot_trees",
    "HeaderResult", "PackChecker", "ParsedHeaders", "RepairReport", "index_checked",
    "parse_headers", "read_headers", "repair_index",
    "RepairPlan", "RepairResult", "RepairSnapshotsOptions", "apply_repair", "plan_repair",
    "repair_snapshots",
]
