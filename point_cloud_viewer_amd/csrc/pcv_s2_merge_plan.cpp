// pcv_s2_merge_plan.cpp — the merge plan of pcv_s2_merge_plan.h. Plain C++.
#include "pcv_s2_merge_plan.h"

#include <algorithm>

namespace {
// the union of the parts' ascending id lists: pairwise std::set_union up a tree (lists that overlap shrink on the way)
std::vector<uint64_t> merged_ids(const PcvS2MergePart* parts, uint32_t num_parts) {
  std::vector<std::vector<uint64_t>> lists;
  lists.reserve(num_parts);
  for (uint32_t p = 0; p < num_parts; ++p)
    if (parts[p].num_cells) lists.emplace_back(parts[p].ids, parts[p].ids + parts[p].num_cells);
  while (lists.size() > 1) {
    std::vector<std::vector<uint64_t>> next;
    next.reserve((lists.size() + 1) / 2);
    for (size_t k = 0; k + 1 < lists.size(); k += 2) {
      std::vector<uint64_t> u(lists[k].size() + lists[k + 1].size());
      u.resize((size_t)(std::set_union(lists[k].begin(), lists[k].end(), lists[k + 1].begin(), lists[k + 1].end(), u.begin()) - u.begin()));
      next.push_back(std::move(u));
    }
    if (lists.size() & 1) next.push_back(std::move(lists.back()));
    lists.swap(next);
  }
  return lists.empty() ? std::vector<uint64_t>() : std::move(lists[0]);
}
}  // namespace

int pcv_s2_merge_plan(const PcvS2MergePart* parts, uint32_t num_parts, uint32_t chunk_points, PcvS2MergePlan* plan, std::string* why) {
  *plan = PcvS2MergePlan();
  if (chunk_points == 0) {
    *why = "chunk_points is 0";
    return PCV_E_INVALID;
  }
  if (num_parts && !parts) {
    *why = "parts is null";
    return PCV_E_INVALID;
  }
  uint64_t total_cells = 0;
  for (uint32_t p = 0; p < num_parts; ++p) {
    if (parts[p].num_cells && (!parts[p].ids || !parts[p].counts)) {
      *why = "part " + std::to_string(p) + ": null ids or counts";
      return PCV_E_INVALID;
    }
    total_cells += parts[p].num_cells;
  }
  // validation first: nothing below has to look at a malformed part
  for (uint32_t p = 0; p < num_parts; ++p) {
    uint64_t at = 0;
    for (uint64_t k = 0; k < parts[p].num_cells; ++k) {
      const uint64_t id = parts[p].ids[k], count = parts[p].counts[k];
      if (id == 0) {
        *why = "part " + std::to_string(p) + ": cell " + std::to_string(k) + " is 0, which is no cell id";
        return PCV_E_INVALID;
      }
      if (k > 0 && id <= parts[p].ids[k - 1]) {
        *why = "part " + std::to_string(p) + ": the cells of a part must ascend by id: cell " + std::to_string(k) + " is not above its predecessor";
        return PCV_E_INVALID;
      }
      if (count == 0) {
        *why = "part " + std::to_string(p) + ": cell " + std::to_string(k) + " holds no points";
        return PCV_E_INVALID;
      }
      if (count >= 0xffffffffull - at) {
        *why = "part " + std::to_string(p) + " holds 2^32 - 1 points or more";
        return PCV_E_INVALID;
      }
      at += count;
    }
  }
  plan->ids = merged_ids(parts, num_parts);
  const size_t cells = plan->ids.size();
  // every part cell's index in the merged list: a walk of the two ascending lists for a part that holds a good share of the
  // cells, a binary search per cell for a small one
  std::vector<uint64_t> rank(total_cells);
  std::vector<uint64_t> first_segment(cells + 1, 0);  // segments per merged cell, then their exclusive scan
  plan->counts.assign(cells, 0);
  {
    size_t e = 0;
    for (uint32_t p = 0; p < num_parts; ++p) {
      const uint64_t k_cells = parts[p].num_cells;
      size_t log2_cells = 1;
      while ((size_t(1) << log2_cells) < cells) ++log2_cells;
      const bool walk = k_cells * log2_cells > cells;
      size_t r = 0;
      for (uint64_t k = 0; k < k_cells; ++k, ++e) {
        const uint64_t id = parts[p].ids[k];
        if (walk) {
          while (plan->ids[r] < id) ++r;
        } else {
          r = (size_t)(std::lower_bound(plan->ids.begin() + r, plan->ids.end(), id) - plan->ids.begin());
        }
        rank[e] = r;
        first_segment[r + 1] += 1;
        plan->counts[r] += parts[p].counts[k];
      }
    }
  }
  for (size_t c = 0; c < cells; ++c) first_segment[c + 1] += first_segment[c];
  plan->offsets.resize(cells);
  uint64_t at = 0;
  for (size_t c = 0; c < cells; ++c) {
    plan->offsets[c] = at;
    at += plan->counts[c];
  }
  // the parts in their order drop their cells into the cells' segment ranges: by cell, then by part
  plan->segments.resize(total_cells);
  {
    std::vector<uint64_t> cursor(first_segment.begin(), first_segment.end() - 1);
    size_t e = 0;
    for (uint32_t p = 0; p < num_parts; ++p) {
      uint64_t src = 0;
      for (uint64_t k = 0; k < parts[p].num_cells; ++k, ++e) {
        pcv_s2_merge_segment& seg = plan->segments[cursor[rank[e]]++];
        seg.dst_offset = 0, seg.src_offset = src, seg.part = p, seg.count = (uint32_t)parts[p].counts[k];
        src += parts[p].counts[k];
      }
    }
  }
  uint64_t dst = 0;
  for (pcv_s2_merge_segment& seg : plan->segments) {
    seg.dst_offset = dst;
    dst += seg.count;
  }
  plan->n = at;
  const uint64_t chunks = (at + chunk_points - 1) / chunk_points;
  plan->chunk_first_segment.resize(chunks);
  uint64_t s = 0;
  for (uint64_t c = 0; c < chunks; ++c) {
    const uint64_t point = c * chunk_points;
    while (s + 1 < plan->segments.size() && plan->segments[s + 1].dst_offset <= point) ++s;
    plan->chunk_first_segment[c] = s;
  }
  return PCV_OK;
}
