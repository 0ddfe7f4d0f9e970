// Host side of todhip_db_select_objects (db_select.hip), plain C++ without HIP so that it can be driven by a stand-alone, sanitized
// host program (tests/db_select_host_test.cpp): the selection as a sorted list of distinct object indices, the view's prefix
// tables, and the view row -> global row search the device kernels restate. The reference's counterpart is the list of object ids
// DescriptorMatcher::parameter_callback is handed (detector.py json_object_ids); it has no such tables.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

// The view of one shard: its selected objects in ascending order. Segment j is one selected object that owns rows of the shard (an
// empty object is selected and counted, but owns no view row and gets no segment).
struct TodViewTables {
  std::vector<uint32_t> objs;           // all distinct selected object indices, ascending (whatever shard holds them)
  std::vector<uint32_t> seg_obj;        // segment j -> full-DB object index
  std::vector<uint32_t> seg_view;       // segment j -> first view row; n_segs + 1 entries, the last one = view rows
  std::vector<uint32_t> seg_global;     // segment j -> first row in the full DB
  uint64_t selected_rows = 0;           // rows of the selected objects in the whole DB
  uint32_t view_rows() const { return seg_view.empty() ? 0u : seg_view.back(); }
  uint32_t n_segs() const { return (uint32_t)seg_obj.size(); }
};

// false: an index >= n_objs (nothing is written then). obj_off: n_objs + 1 prefix sums of the objects' row counts. Shards are
// object-aligned and contiguous (todhip_db_load), so an object with rows is the shard's iff its first row lies in
// [shard_first, shard_first + shard_rows).
inline bool tod_view_build(const uint32_t* ids, uint32_t n_ids, const uint32_t* obj_off, uint32_t n_objs, uint64_t shard_first,
                           uint64_t shard_rows, TodViewTables* out) {
  for (uint32_t i = 0; i < n_ids; ++i)
    if (ids[i] >= n_objs) return false;
  TodViewTables t;
  t.objs.assign(ids, ids + n_ids);
  std::sort(t.objs.begin(), t.objs.end());
  t.objs.erase(std::unique(t.objs.begin(), t.objs.end()), t.objs.end());
  uint32_t view = 0;
  for (uint32_t o : t.objs) {
    const uint32_t lo = obj_off[o], n = obj_off[o + 1] - lo;
    t.selected_rows += n;
    if (n == 0 || lo < shard_first || lo >= shard_first + shard_rows) continue;   // not this shard's rows
    t.seg_obj.push_back(o);
    t.seg_view.push_back(view);
    t.seg_global.push_back(lo);
    view += n;
  }
  t.seg_view.push_back(view);
  *out = std::move(t);
  return true;
}

// The segment of view row r (< view rows): the last j with seg_view[j] <= r. The kernels of db_select.hip run the same loop.
inline uint32_t tod_view_segment(const uint32_t* seg_view, uint32_t n_segs, uint32_t r) {
  uint32_t lo = 0, hi = n_segs;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg_view[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

inline uint32_t tod_view_to_global(const TodViewTables& t, uint32_t r) {
  const uint32_t j = tod_view_segment(t.seg_view.data(), t.n_segs(), r);
  return t.seg_global[j] + (r - t.seg_view[j]);
}
