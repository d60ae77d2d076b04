"""The knobs of rtKernelSetTuning as include/rt_hip.h documents them: (name in N.TUNING, default,
lowest, highest, required multiple).  Written out here, never read from the library's table, so the
tests that use it (test_tuning.py on the CPU, test_gpu_state.py through the C ABI) pin that table."""
INT_MAX = 2 ** 31 - 1

KNOBS = [
    ("refill_min", 6, 1, 64, 1),
    ("shade_min", 48, 1, 64, 1),
    ("refill_min_global", 0, 0, 64, 1),
    ("shade_min_global", 0, 0, 64, 1),
    ("step_weight_node", 35, 1, 1000, 1),
    ("step_weight_leaf", 55, 1, 1000, 1),
    ("step_weight_node_global", 0, 0, 1000, 1),
    ("step_weight_leaf_global", 0, 0, 1000, 1),
    ("chunk_pixels", 0, 0, 4096, 64),
    ("tail_chunk", 256, 64, 4096, 64),
    ("bulk_percent", 80, 0, 100, 1),
    ("tile_major", -1, -1, 2, 1),
    ("max_blocks", 0, 0, 64, 1),
    ("perframe_sky", 1, 0, 2, 1),
    ("wf_refill_min", 32, 1, 64, 1),
    ("wf_streams_per_cu", 0, 0, 64, 1),
    ("wf_top_nodes", 256, 0, 1024, 1),
    ("global_oct", 1, 0, 1, 1),
    ("perframe_defer", 2, 0, 2, 1),
    ("perframe_defer_min", 4194304, 0, INT_MAX, 1),
    ("perframe_batch", 8, 1, 8, 1),
    ("query_refill_min", 32, 1, 64, 1),
]
# kept with the packed scene it renumbers, outside the table: checked through the C ABI only
TOP_NODES = ("top_nodes", 384, 0, 1024, 1)
# ids the C ABI refuses: the retired ones, and the two either side of the enum
REFUSED_IDS = (10, 11, 12, 22, -1, 27)
