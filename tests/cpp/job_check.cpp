// Host check of rt_wavefront.hpp's wf_job_valid (tests/test_job_host.py): the
// rules of a render job as a table of cases, the same cases and a sweep of
// every rule's neighbourhood against `old_rules` (the checks Wavefront::render
// made on its positional arguments before WfJob carried them), and the size
// of the kernels' argument block.
#include <cstdio>

#include "rt_wavefront.hpp"

using namespace rtamd;

static bool old_rules(bool camera_mode, unsigned n0, unsigned aa, unsigned max_depth, unsigned blk_period,
                      unsigned long long blk_mask, const FrameTable* batch, unsigned n_frames) {
  if (max_depth + 2 > (unsigned)kMaxGen) return false;
  if (blk_period > 64 || (blk_period && (blk_mask == 0 || (blk_period < 64 && (blk_mask >> blk_period) != 0))))
    return false;
  if (aa == 0 || aa > 16 || (aa & (aa - 1)) != 0 || (!camera_mode && aa != 1) || n0 % aa != 0) return false;
  if (n_frames == 0 || n_frames > kMaxFrames || (n_frames > 1 && !batch)) return false;
  return true;
}
static bool old_rules(const WfJob& j) {
  return old_rules(j.d_in_rays == nullptr, j.n0, j.aa, j.max_depth, j.blk_period, j.blk_mask, j.batch, j.n_frames);
}

static int n_bad = 0;
static void expect(const char* what, const WfJob& j, bool ok) {
  if (wf_job_valid(j) == ok && old_rules(j) == ok) return;
  std::printf("FAIL %s: expected %d, wf_job_valid %d, old rules %d\n", what, (int)ok, (int)wf_job_valid(j),
              (int)old_rules(j));
  ++n_bad;
}

int main() {
  static_assert(sizeof(WfArgs) == 336, "WfArgs");
  if (sizeof(WfArgs) != 336) {
    std::printf("FAIL sizeof(WfArgs) %zu\n", sizeof(WfArgs));
    return 1;
  }
  static FrameTable tab{};
  static const double rays[12] = {};
  double out[6];
  const DevCamera cam{};
  auto camera = [&](unsigned aa) { return WfJob::camera_shard(cam, 64 * aa, aa, 5, out, 8); };

  for (unsigned aa : {1u, 2u, 4u, 8u, 16u}) expect("camera aa", camera(aa), true);
  for (unsigned aa : {0u, 3u, 32u}) {
    WfJob j = camera(1);
    j.aa = aa;
    j.n0 = 96;  // divisible by 3 and 32: only the sample count is at fault
    expect("camera bad aa", j, false);
  }
  {
    WfJob j = WfJob::ray_batch(rays, 2, 5, out);
    expect("ray batch", j, true);
    j.aa = 2;
    expect("ray batch aa 2", j, false);
  }
  {
    WfJob j = camera(4);
    j.n0 = 66;
    expect("n0 % aa", j, false);
  }
  {
    WfJob j = camera(1);
    j.max_depth = 64;
    expect("max_depth 64", j, true);
    j.max_depth = 65;
    expect("max_depth 65", j, false);
  }
  struct Pat {
    unsigned period;
    unsigned long long mask;
    bool ok;
  };
  const Pat pats[] = {{0, 0ull, true},      {0, ~0ull, true},    {0, 0x100ull, true}, {65, 1ull, false},
                      {8, 0ull, false},     {8, 0x100ull, false}, {8, 0xFFull, true},  {64, ~0ull, true}};
  for (const Pat& p : pats) {
    WfJob j = WfJob::block_pattern(cam, 64, 1, 5, out, 8, p.period, p.mask);
    expect("pattern", j, p.ok);
  }
  {
    WfJob j = camera(1);
    j.n_frames = 0;
    expect("n_frames 0", j, false);
    j.n_frames = 17;
    j.batch = &tab;
    expect("n_frames 17", j, false);
    j.n_frames = 2;
    j.batch = nullptr;
    expect("n_frames 2, no table", j, false);
    j.batch = &tab;
    expect("n_frames 2", j, true);
  }

  // every rule's neighbourhood: the function and the old checks agree everywhere
  const unsigned long long masks[] = {0ull, 1ull, 0xFFull, 0x100ull, 1ull << 63, ~0ull};
  long n_cases = 0;
  for (int mode = 0; mode < 2; ++mode)
    for (unsigned aa = 0; aa <= 33; ++aa)
      for (unsigned n0 : {0u, 1u, 64u, 96u, 66u})
        for (unsigned depth : {0u, 63u, 64u, 65u, 1000u})
          for (unsigned period : {0u, 1u, 8u, 63u, 64u, 65u, 200u})
            for (unsigned long long mask : masks)
              for (unsigned nf : {0u, 1u, 2u, 16u, 17u})
                for (int with_tab = 0; with_tab < 2; ++with_tab) {
                  WfJob j = mode ? WfJob::ray_batch(rays, n0, depth, out)
                                 : WfJob::block_pattern(cam, n0, aa, depth, out, 8, period, mask);
                  j.aa = aa;
                  j.blk_period = period;
                  j.blk_mask = mask;
                  j.n_frames = nf;
                  j.batch = with_tab ? &tab : nullptr;
                  ++n_cases;
                  if (wf_job_valid(j) != old_rules(j)) {
                    if (n_bad < 10)
                      std::printf("FAIL sweep mode %d aa %u n0 %u depth %u period %u mask %llx frames %u table %d\n",
                                  mode, aa, n0, depth, period, mask, nf, with_tab);
                    ++n_bad;
                  }
                }
  if (n_bad) return 1;
  std::printf("OK %ld cases\n", n_cases);
  return 0;
}
