"""wcg - MI355X-native word count for the Lab 1 MapReduce hot path of wushan270/mit-6.824-2015.

Python host side (tests, bench, multi-GPU orchestration) over the C ABI of libwcg.so
(include/wcg.h).  The compute path is hand-written HIP for gfx950; there is no CPU fallback.
"""
from ._lib import (Engine, WcgError, ihash, load, version, EXPORTED, RECORD_BYTES,  # noqa: F401
                   exchange_plan, gather_plan, exchange_local, gather_merge_local,
                   top_of_merged, top_merge, TOP_MAX,
                   lookup_in_merged, range_of_merged, prefix_succ, check_merged, MERGED_KINDS,
                   JSON_MAP, JSON_RES,
                   by_count_of_merged, count_rank_of_merged, by_count_merge)
