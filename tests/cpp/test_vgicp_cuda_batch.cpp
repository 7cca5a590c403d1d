// fast_gicp::LoopVerifierHip with setVGICPCuda (riv-slam_amd/cpp/loop_verifier_hip.hpp): FAST_VGICP_CUDA on the batch handle through the C ABI.
//   test_vgicp_cuda_batch                     compile-and-link check (no GPU needed)
//   test_vgicp_cuda_batch set.bin out.bin     set.bin: int32 n_candidates, int32 n_tgt, int32 n_src[n_candidates], float guesses[n_candidates][16]
//                                             (column-major), tgt xyz[n_tgt * 3], then every candidate's xyz[n_src * 3].
//                                             The verifier registers every candidate against the target in one batch in this mode (DIRECT_RADIUS 1.5,
//                                             resolution 1.0, PLANE, default parameters).  out.bin: the batch's apdgicp_result records, then the
//                                             scores (double), then int64 {clouds prepared, maps built, preparation waits, map waits}.
//                                             Prints "<best> <setVGICPCuda(GPU_RBF_KERNEL) refused and the mode kept> <the other modes off>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "loop_verifier_hip.hpp"

int main(int argc, char** argv) {
  apdgicp_params p;
  apdgicp_default_params(&p);
  apdgicp_vgicp_cuda_params vp;
  apdgicp_vgicp_cuda_default_params(&vp);
  vp.neighbor_search = APDGICP_VGICP_CUDA_DIRECT_RADIUS;
  vp.search_radius = 1.5;
  if (argc < 3) {
    fast_gicp::LoopVerifierHip v(&p);  // (without a GPU: one line on stderr, ok() == false)
    std::printf("compile-only %d\n", v.ok() ? v.setVGICPCuda(&vp) : 0);
    return 0;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int head[2];
  if (std::fread(head, 4, 2, f) != 2) return 2;
  const int nc = head[0], nt = head[1];
  std::vector<int> ns((size_t)nc);
  if (std::fread(ns.data(), 4, ns.size(), f) != ns.size()) return 2;
  std::vector<float> guesses(16 * (size_t)nc), t(3 * (size_t)nt);
  if (std::fread(guesses.data(), 4, guesses.size(), f) != guesses.size() || std::fread(t.data(), 4, t.size(), f) != t.size()) return 2;
  std::vector<std::vector<float>> s((size_t)nc);
  for (int i = 0; i < nc; i++) {
    s[(size_t)i].resize(3 * (size_t)ns[(size_t)i]);
    if (std::fread(s[(size_t)i].data(), 4, s[(size_t)i].size(), f) != s[(size_t)i].size()) return 2;
  }
  std::fclose(f);
  const double max_range = std::numeric_limits<double>::max(), thresh = 5.0;

  fast_gicp::LoopVerifierHip verifier(&p);
  if (!verifier.ok()) return 3;
  apdgicp_vgicp_params other;
  apdgicp_vgicp_default_params(&other);
  if (verifier.setVGICP(&other) != 0) return 3;  // switched off again by the next call
  if (verifier.setVGICPCuda(&vp) != 0) return 3;
  apdgicp_vgicp_cuda_params bad = vp;
  bad.nn_method = APDGICP_NN_GPU_RBF_KERNEL;
  int refused = verifier.setVGICPCuda(&bad) == APDGICP_ERR_UNSUPPORTED;
  apdgicp_vgicp_cuda_params now;
  int on = 0, vg_on = 1, nd_on = 1, ic_on = 1;
  if (apdgicp_batch_get_vgicp_cuda(verifier.handle(), &now, &on) != 0) return 3;
  refused &= on == 1 && now.nn_method == vp.nn_method && now.neighbor_search == vp.neighbor_search && now.search_radius == vp.search_radius;
  if (apdgicp_batch_get_vgicp(verifier.handle(), nullptr, &vg_on) != 0 || apdgicp_batch_get_ndt(verifier.handle(), nullptr, &nd_on) != 0 ||
      apdgicp_batch_get_icp(verifier.handle(), nullptr, &ic_on) != 0)
    return 3;
  std::vector<fast_gicp::LoopCloud> cands;
  for (int i = 0; i < nc; i++) cands.push_back(fast_gicp::LoopCloud{s[(size_t)i].data(), ns[(size_t)i], 12});
  fast_gicp::LoopMatch m;
  if (verifier.matching(fast_gicp::LoopCloud{t.data(), nt, 12}, cands, guesses.data(), max_range, thresh, &m) != 0) {
    std::fprintf(stderr, "matching failed: %s\n", apdgicp_last_error());
    return 4;
  }
  int64_t counts[4] = {0, 0, 0, 0};
  if (apdgicp_batch_vgicp_cuda_build_count(verifier.handle(), &counts[0], &counts[1]) != 0 ||
      apdgicp_batch_vgicp_cuda_debug_counts(verifier.handle(), &counts[2], &counts[3], nullptr) != 0)
    return 4;
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  std::fwrite(m.results.data(), sizeof(apdgicp_result), m.results.size(), o);
  std::fwrite(m.scores.data(), sizeof(double), m.scores.size(), o);
  std::fwrite(counts, sizeof(int64_t), 4, o);
  std::fclose(o);
  std::printf("%d %d %d\n", m.best, refused, (vg_on || nd_on || ic_on) ? 0 : 1);
  return 0;
}
