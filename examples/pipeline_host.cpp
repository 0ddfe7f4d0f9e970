// A C++ host of the detection pipeline: todhip.h and the standard library, nothing else.
//
//   g++ -std=c++17 -Iinclude examples/pipeline_host.cpp -Ltod_amd -ltodhip -Wl,-rpath,$PWD/tod_amd -o pipeline_host
//   GPU_MAX_HW_QUEUES=8 ./pipeline_host            ("Streams and hardware queues")
//   GPU_MAX_HW_QUEUES=8 ./pipeline_host --objects 3,1   look for objects 3 and 1 only (the reference detector's json_object_ids)
//
// It creates a pipeline, loads an object DB from plain arrays, keeps ring_depth batches in flight -- it submits ahead and waits for
// the oldest ticket only when the ring is full -- and prints the poses. The frames here are noise and the DB is random, so it prints
// no pose; a real host puts its camera frames and its trained models (todhip_model_*, or rows read from its database) in their place.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

#include "todhip.h"

namespace {

struct Batch { std::vector<uint8_t> gray; std::vector<float> depth; };

// One ticket's results, printed.
int drain(todhip_pipeline* pipe, uint64_t ticket, uint32_t n_frames, uint32_t n_features) {
  std::vector<uint32_t> n_kp(n_frames), pose_ptr(n_frames + 1), inliers(n_frames * 16 * n_features);
  std::vector<todhip_pose> poses(n_frames * 16);
  for (;;) {
    uint32_t n_poses = (uint32_t)poses.size(), n_inl = (uint32_t)inliers.size();
    const int rc = todhip_pipeline_wait(pipe, ticket, 0, n_kp.data(), nullptr, poses.data(), &n_poses, pose_ptr.data(), inliers.data(), &n_inl);
    if (rc == TODHIP_ECAPACITY) {                       // the needed counts came back and the ticket is still there: make room, ask again
      poses.resize(n_poses); inliers.resize(n_inl);
      continue;
    }
    if (rc != TODHIP_OK) { std::fprintf(stderr, "ticket %llu: todhip_status %d\n", (unsigned long long)ticket, rc); return rc; }
    for (uint32_t f = 0; f < n_frames; ++f) {
      std::printf("ticket %llu frame %u: %u keypoints, %u poses\n", (unsigned long long)ticket, f, n_kp[f], pose_ptr[f + 1] - pose_ptr[f]);
      for (uint32_t i = pose_ptr[f]; i < pose_ptr[f + 1]; ++i)
        std::printf("  object %u  t = (%.4f %.4f %.4f)  %u inliers\n", poses[i].object, poses[i].t[0], poses[i].t[1], poses[i].t[2],
                    poses[i].inlier_end - poses[i].inlier_begin);
    }
    return TODHIP_OK;
  }
}

}  // namespace

int main(int argc, char** argv) {
  // --objects a,b,c: indices into the objs[] loaded below; without it every object is searched
  std::vector<uint32_t> wanted;
  bool restrict_objects = false;
  for (int a = 1; a < argc; ++a) {
    if (std::strcmp(argv[a], "--objects") != 0 || a + 1 >= argc) { std::fprintf(stderr, "usage: %s [--objects 3,17,42]\n", argv[0]); return 2; }
    restrict_objects = true;
    for (const char* p = argv[++a]; *p;) {
      char* end = nullptr;
      wanted.push_back((uint32_t)std::strtoul(p, &end, 10));
      if (end == p) { std::fprintf(stderr, "--objects: a comma-separated list of object indices\n"); return 2; }
      p = *end == ',' ? end + 1 : end;
    }
  }

  todhip_pipeline_params prm;
  todhip_pipeline_default_params(&prm);                 // struct_size and the defaults; then what this host knows
  prm.frames_per_step = 8;
  prm.H = 480; prm.W = 640;
  const float K[9] = {525.f, 0.f, 320.f, 0.f, 525.f, 240.f, 0.f, 0.f, 1.f};
  for (int i = 0; i < 9; ++i) prm.K9[i] = K[i];
  prm.n_features = 500;
  prm.ring_depth = 3;

  todhip_pipeline* pipe = nullptr;
  int rc = todhip_pipeline_create(0, &prm, &pipe);
  if (rc != TODHIP_OK) { std::fprintf(stderr, "todhip_pipeline_create: todhip_status %d\n", rc); return 1; }

  // the object DB from arrays: per object n descriptors of 32 bytes and n model points
  std::mt19937 gen(1);
  const uint32_t n_objs = 4, rows = 2000;
  std::vector<std::vector<uint8_t>> desc(n_objs, std::vector<uint8_t>(rows * 32));
  std::vector<std::vector<float>> pts(n_objs, std::vector<float>(rows * 3));
  std::vector<todhip_object> objs(n_objs);
  for (uint32_t o = 0; o < n_objs; ++o) {
    for (uint8_t& b : desc[o]) b = (uint8_t)gen();
    for (float& v : pts[o]) v = (float)(gen() % 1000) * 1e-4f;
    objs[o].desc = desc[o].data(); objs[o].pts_xyz = pts[o].data(); objs[o].n = rows;
  }
  rc = todhip_pipeline_db_load(pipe, objs.data(), n_objs, 32);
  if (rc != TODHIP_OK) { std::fprintf(stderr, "todhip_pipeline_db_load: todhip_status %d\n", rc); todhip_pipeline_destroy(pipe); return 1; }

  if (restrict_objects) {                                // between steps only: TODHIP_EBUSY while a ticket is outstanding
    rc = todhip_pipeline_select_objects(pipe, wanted.data(), (uint32_t)wanted.size());
    if (rc != TODHIP_OK) { std::fprintf(stderr, "todhip_pipeline_select_objects: todhip_status %d\n", rc); todhip_pipeline_destroy(pipe); return 1; }
    uint32_t n_sel = 0; uint64_t sel_rows = 0;
    todhip_db_selection(todhip_pipeline_matcher(pipe), &n_sel, &sel_rows, nullptr);
    std::printf("searching %u of %u objects, %llu rows\n", n_sel, n_objs, (unsigned long long)sel_rows);
  }

  const uint32_t B = prm.frames_per_step, n_batches = 6;
  const size_t px = (size_t)prm.H * prm.W;
  Batch batch;                                           // one host buffer serves every submit: it is free again when submit returns
  batch.gray.resize(B * px); batch.depth.assign(B * px, 0.8f);

  std::deque<uint64_t> in_flight;
  int failed = 0;
  for (uint32_t b = 0; b < n_batches && !failed; ++b) {
    for (uint8_t& v : batch.gray) v = (uint8_t)gen();    // "the next camera frames"
    uint64_t ticket = 0;
    while ((rc = todhip_pipeline_submit(pipe, batch.gray.data(), batch.depth.data(), B, &ticket)) == TODHIP_EBUSY) {
      failed = drain(pipe, in_flight.front(), B, prm.n_features) != TODHIP_OK;   // the ring is full: take the oldest results
      in_flight.pop_front();
      if (failed) break;
    }
    if (failed || rc != TODHIP_OK) { failed = 1; break; }
    in_flight.push_back(ticket);
  }
  for (; !in_flight.empty() && !failed; in_flight.pop_front()) failed = drain(pipe, in_flight.front(), B, prm.n_features) != TODHIP_OK;

  todhip_pipeline_stats st;
  if (todhip_pipeline_get_stats(pipe, &st) == TODHIP_OK)
    std::printf("%llu steps, %llu frames, %llu keypoints, %llu poses; host seconds: orb %.3f, match issue %.3f, verify %.3f\n",
                (unsigned long long)st.steps, (unsigned long long)st.frames, (unsigned long long)st.keypoints, (unsigned long long)st.poses,
                st.orb_s, st.match_issue_s, st.verify_s);
  todhip_pipeline_destroy(pipe);                         // (would also drain tickets that nobody waited for)
  return failed;
}
