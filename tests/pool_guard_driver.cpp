// Stand-alone driver of csrc/pcv_pool_guard.h, the layout arithmetic of the device pool's guard mode (built by
// test_pool_guard_cpu.py with -fsanitize=address,undefined; no library involved). argv[1] is a file of cases, one per line:
// `requested block_bytes fill` (block_bytes 0: what the request asks the pool for; larger: a block the cache's loose match
// handed out). A block is a heap array of exactly block_bytes, so a scan that leaves it is the sanitizer's to report.
// Per case the driver prints
//   case <requested> <block_bytes> <fill>
//   layout <block_bytes> <user_off> <back_off> <back_bytes> <canary>
//   painted <first index that is neither fence nor fill, or -1>
//   damage <where> <byte written, relative to the user pointer> <reported offset | none>
// for <where> in none, front_first, front_last, back_first, back_last, both.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>

#include "../point_cloud_viewer_amd/csrc/pcv_pool_guard.h"

static void report(const char* where, int64_t planted, const uint8_t* block, const PcvGuardLayout& lay, uint8_t canary) {
  int64_t off = 0;
  if (pcv_guard_first_damage(block, block + lay.back_off, lay, canary, &off))
    std::printf("damage %s %" PRId64 " %" PRId64 "\n", where, planted, off);
  else
    std::printf("damage %s %" PRId64 " none\n", where, planted);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    uint64_t requested = 0, block_bytes = 0;
    unsigned fill_in = 0;
    if (!(ss >> requested >> block_bytes >> fill_in)) continue;
    const uint8_t fill = (uint8_t)fill_in, canary = pcv_guard_canary(fill);
    if (block_bytes == 0) block_bytes = pcv_guard_block_request(requested);
    std::printf("case %" PRIu64 " %" PRIu64 " %u\n", requested, block_bytes, fill_in);
    PcvGuardLayout lay;
    if (!pcv_guard_layout(requested, block_bytes, &lay)) {
      std::printf("layout too-small\n");
      continue;
    }
    std::printf("layout %zu %zu %zu %zu %u\n", lay.block_bytes, lay.user_off, lay.back_off, lay.back_bytes, (unsigned)canary);
    std::unique_ptr<uint8_t[]> block(new uint8_t[block_bytes]);
    // painted the way the pool paints it: front fence, the caller's bytes, back fence
    std::memset(block.get(), canary, lay.user_off);
    std::memset(block.get() + lay.user_off, fill, requested);
    std::memset(block.get() + lay.back_off, canary, lay.back_bytes);
    int64_t bad = -1;
    for (size_t i = 0; i < block_bytes && bad < 0; ++i) {
      const bool user = i >= lay.user_off && i < lay.user_off + requested;
      if (block[i] != (user ? fill : canary)) bad = (int64_t)i;
    }
    if (bad < 0 && pcv_guard_first_unfilled(block.get() + lay.user_off, requested, fill) >= 0) bad = (int64_t)lay.user_off;
    std::printf("painted %" PRId64 "\n", bad);

    uint8_t* user = block.get() + lay.user_off;
    const int64_t front_first = -(int64_t)lay.user_off, front_last = -1;
    const int64_t back_first = (int64_t)requested, back_last = (int64_t)(block_bytes - lay.user_off) - 1;
    report("none", 0, block.get(), lay, canary);
    const struct {
      const char* where;
      int64_t at;
    } spots[] = {{"front_first", front_first}, {"front_last", front_last}, {"back_first", back_first}, {"back_last", back_last}};
    for (const auto& s : spots) {
      const uint8_t keep = user[s.at];
      user[s.at] = (uint8_t)(canary ^ 0x01);  // one bit: the scan compares whole bytes
      report(s.where, s.at, block.get(), lay, canary);
      user[s.at] = keep;
    }
    user[back_last] = fill;
    user[front_last] = fill;
    report("both", front_last, block.get(), lay, canary);  // the front fence is looked at first
    // a write of the caller's own last byte is no damage
    user[back_last] = canary;
    user[front_last] = canary;
    if (requested) user[requested - 1] = (uint8_t)~fill;
    report("own_last", (int64_t)requested - 1, block.get(), lay, canary);
  }
  return 0;
}
