// adapter/ecto_cells.hpp's DescriptorMatcher cell on 64-byte descriptors (BRISK, FREAK, AKAZE padded), against the mini_ecto test
// double, the way tests/adapter_test.cpp drives the cell on 32-byte ones.
//   adapter_wide_test <dir> declare-only   the cell's declarations compile and carry the reference's names
//   adapter_wide_test <dir> cpu            load_models refuses mixed widths and a width of 48 by object name, before any library call
//                                          (no GPU is touched: the cell is never configured)
//   adapter_wide_test <dir>                <dir>/{desc,pts,obj_off,q_desc}.bin: 64-byte models and one frame through the cell; the matches
//                                          go to <dir>/out_matches.bin / out_dist.bin; then a 32-column query must throw
#include "mini_ecto/mini_ecto.hpp"
#include "../adapter/ecto_cells.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>

template <typename T> static std::vector<T> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw std::runtime_error("cannot open " + path);
  const size_t n = (size_t)f.tellg();
  std::vector<T> v(n / sizeof(T));
  f.seekg(0);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  return v;
}
template <typename T> static void dump(const std::string& path, const std::vector<T>& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

typedef tod_amd::DescriptorMatcher::ObjectModel Model;

static Model model(const std::string& id, int n, int cols, int type = CV_8U) {
  Model m;
  m.id = id;
  m.descriptors = cv::Mat(n, cols, type);
  m.points = cv::Mat(n, 1, CV_32FC3);
  return m;
}

// what load_models throws for these documents ("" when it does not throw)
static std::string refusal(const std::vector<Model>& docs) {
  tod_amd::DescriptorMatcher cell;                            // not configured: a refusal must come before the library is asked
  try { cell.load_models(docs); } catch (const std::runtime_error& e) { return e.what(); }
  return "";
}

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "usage: adapter_wide_test <dir> [declare-only | cpu]\n"; return 2; }
  const std::string dir = argv[1], mode = argc > 2 ? argv[2] : "";
  try {
    ecto::tendrils mp, mi, mo;
    tod_amd::DescriptorMatcher::declare_params(mp);
    tod_amd::DescriptorMatcher::declare_io(mp, mi, mo);
    if (!mp.has("search_json_params") || !mi.has("descriptors") || !mo.has("matches") || !mo.has("matches_3d") || !mo.has("object_ids") ||
        !mo.has("spans")) return 3;
    if (mode == "declare-only") { std::cout << "declare ok\n"; return 0; }

    if (mode == "cpu") {
      // mixed widths: the first object whose width differs is named, whichever way round
      std::string what = refusal({model("obj_a", 10, 32), model("obj_b", 0, 0), model("obj_c", 7, 64)});
      if (what.find("obj_c") == std::string::npos) { std::cerr << "mixed 32/64: '" << what << "'\n"; return 4; }
      what = refusal({model("obj_a", 10, 64), model("obj_b", 3, 32)});
      if (what.find("obj_b") == std::string::npos) { std::cerr << "mixed 64/32: '" << what << "'\n"; return 4; }
      // a width the library does not search, and a type that is not bytes
      what = refusal({model("obj_a", 10, 48)});
      if (what.find("obj_a") == std::string::npos) { std::cerr << "width 48: '" << what << "'\n"; return 5; }
      what = refusal({model("obj_a", 5, 64), model("obj_f", 10, 64, CV_32F)});
      if (what.find("obj_f") == std::string::npos) { std::cerr << "CV_32F: '" << what << "'\n"; return 5; }
      std::cout << "cpu ok\n";
      return 0;
    }

    // ---- 64-byte models and one frame through the cell
    mp["search_json_params"] << std::string("{\"type\": \"LSH\", \"radius\": 70}");
    tod_amd::DescriptorMatcher matcher;
    matcher.configure(mp, mi, mo);
    std::vector<uint32_t> off = slurp<uint32_t>(dir + "/obj_off.bin");
    std::vector<uint8_t> desc = slurp<uint8_t>(dir + "/desc.bin");
    std::vector<float> pts = slurp<float>(dir + "/pts.bin");
    std::vector<Model> docs;
    for (size_t o = 0; o + 1 < off.size(); ++o) {
      const int n = (int)(off[o + 1] - off[o]);
      Model m = model("object_" + std::to_string(o), n, n ? 64 : 0);   // an empty model has no width of its own
      if (n) {
        std::memcpy(m.descriptors.ptr<uint8_t>(0), &desc[(size_t)off[o] * 64], (size_t)n * 64);
        std::memcpy(m.points.ptr<float>(0), &pts[(size_t)off[o] * 3], (size_t)n * 12);
      }
      docs.push_back(m);
    }
    matcher.load_models(docs);
    std::vector<uint8_t> q = slurp<uint8_t>(dir + "/q_desc.bin");
    const int nq = (int)(q.size() / 64);
    cv::Mat qm(nq, 64, CV_8U);
    std::memcpy(qm.ptr<uint8_t>(0), q.data(), q.size());
    mi["descriptors"] << qm;
    if (matcher.process(mi, mo) != ecto::OK) return 6;
    const std::vector<std::vector<cv::DMatch> >& matches = mo.get<std::vector<std::vector<cv::DMatch> > >("matches");
    const std::vector<cv::Mat>& m3d = mo.get<std::vector<cv::Mat> >("matches_3d");
    std::vector<int32_t> flat;
    std::vector<float> dist, xyz;
    for (size_t qi = 0; qi < matches.size(); ++qi) {
      for (const cv::DMatch& m : matches[qi]) { flat.push_back(m.queryIdx); flat.push_back(m.trainIdx); flat.push_back(m.imgIdx); dist.push_back(m.distance); }
      if ((size_t)m3d[qi].cols != matches[qi].size()) return 6;
      for (size_t j = 0; j < 3 * matches[qi].size(); ++j) xyz.push_back(m3d[qi].ptr<float>(0)[j]);
    }
    dump(dir + "/out_matches.bin", flat);
    dump(dir + "/out_dist.bin", dist);
    dump(dir + "/out_xyz.bin", xyz);
    // a 32-column query against the 64-byte DB must throw, not be read at the wrong stride
    bool threw = false;
    mi["descriptors"] << cv::Mat(nq, 32, CV_8U);
    try { matcher.process(mi, mo); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) return 7;
    std::cout << "adapter wide ok: " << dist.size() << " matches\n";
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "adapter_wide_test: " << e.what() << "\n";
    return 1;
  }
}
