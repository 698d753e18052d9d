// Headless driver (SURVEY 8(b) caller 1): .cli -> rt_* C ABI -> PNG (+ optional float RGB dump).
// The native counterpart of myRTFileReader's `write` command (myRTFileReader.java:86-93), which
// calls myScene.draw() and saves rndrdImg as PNG (myScene.java:1185-1196).
//
//   rtrender <scene_dir> <file.cli> [-w W] [-h H] [-spp N] [-seed S] [-device D] [-o out.png]
//            [-rgb out.f32] [-tex name=path.ppm]... [-time ITERS] [-nodir] [-budget MS] [-noise E [-max N]]
//            [-denoise [LEVELS]] [-eye X Y Z -at X Y Z [-up X Y Z]]
//
// -budget MS: the best frame MS milliseconds give, in place of -spp's fixed count -- samples are accumulated
// (rt_accum_*) in chunks of 2, 2, 4, 8, ... doubling up to 64 until the wall time since the first chunk was
// issued exceeds MS; prints "samples N" and writes the frame of those N samples.
//
// -noise E [-max N]: samples only where the frame is still noisy (rt_accum_select_error / rt_accum_add_selected).
// Every pixel gets 4 samples; then, until no pixel is selected, the pixels whose standard error exceeds E and
// that have fewer than N samples (default 1024) get 4, 8, 16, ... doubling up to 64 more, a chunk never taking
// a pixel past N. Prints "pixels W*H samples TOTAL max MAXCOUNT" (the samples shaded in all and the largest
// count of a pixel) and writes the resolved frame.
//
// -denoise [LEVELS]: the written frame is the denoised one (rt_denoise_*, the defaults with LEVELS a-trous levels
// if given) instead of the resolved one. With -budget and -noise the accumulator of that mode also keeps the
// moments; with a plain -spp N (N >= 2) the N samples go through a moments accumulator in one add.
//
// -eye X Y Z -at X Y Z [-up X Y Z]: the frame as seen from the eye at X Y Z looking at the point -at, with -up
// (default 0 1 0) upwards, over the scene as the .cli places it (rt_camera_look_at, rt_accum_set_camera). The frame
// is rendered through an accumulator with that pose: it combines with -budget, -noise and -denoise as they are, and
// a plain -spp N (N >= 1, required) adds the N samples in one add and writes the resolved frame. Without -eye every
// path above and its output are as they were.
//
// Without -o the image goes where myScene.saveFile puts it (myScene.java:1185-1196): the
// `write` name (rt_scene_save_name) inside the folder "pics.<yyyy.MM.dd.hh.mm>" the scene
// creates (myScene.java:170, getDateTimeString :1329-1340; saveImgInDir defaults on :182),
// or in the current directory with -nodir. '/' separates the folder (the reference
// concatenates a Windows "\\").
//
// Textures are binary PPM (P6, 8-bit) files, one per texture name the .cli references
// (tools/textures_to_ppm.py converts the scene textures with the same decoder the tests use).
// Build: tools/build_rtrender.sh (links libdistraytracer.so and zlib).
#include <zlib.h>

#include <sys/stat.h>

#include <chrono>
#include <cstdio>
#include <ctime>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/distraytracer.h"

static bool read_ppm(const std::string& path, int& w, int& h, std::vector<uint8_t>& rgb) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  char magic[3] = {0};
  int maxv = 0;
  bool ok = std::fscanf(f, "%2s %d %d %d", magic, &w, &h, &maxv) == 4 && std::strcmp(magic, "P6") == 0 && maxv == 255;
  if (ok) {
    std::fgetc(f);  // single whitespace after the header
    rgb.resize((size_t)w * h * 3);
    ok = std::fread(rgb.data(), 1, rgb.size(), f) == rgb.size();
  }
  std::fclose(f);
  return ok;
}

static void be32(std::vector<uint8_t>& v, uint32_t x) {
  for (int s = 24; s >= 0; s -= 8) v.push_back((uint8_t)(x >> s));
}
static void chunk(FILE* f, const char* type, const std::vector<uint8_t>& data) {
  std::vector<uint8_t> c;
  be32(c, (uint32_t)data.size());
  c.insert(c.end(), type, type + 4);
  c.insert(c.end(), data.begin(), data.end());
  uint32_t crc = crc32(0, c.data() + 4, (uInt)(c.size() - 4));
  be32(c, crc);
  std::fwrite(c.data(), 1, c.size(), f);
}
// PImage.save of rndrdImg: 8-bit RGB from the ARGB ints (myColor.getInt packing)
static bool write_png(const std::string& path, int w, int h, const int32_t* argb) {
  std::vector<uint8_t> raw;
  raw.reserve((size_t)h * (w * 3 + 1));
  for (int y = 0; y < h; ++y) {
    raw.push_back(0);
    for (int x = 0; x < w; ++x) {
      uint32_t p = (uint32_t)argb[(size_t)y * w + x];
      raw.push_back((uint8_t)(p >> 16)); raw.push_back((uint8_t)(p >> 8)); raw.push_back((uint8_t)p);
    }
  }
  uLongf n = compressBound((uLong)raw.size());
  std::vector<uint8_t> z(n);
  if (compress2(z.data(), &n, raw.data(), (uLong)raw.size(), 6) != Z_OK) return false;
  z.resize(n);
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  std::fwrite(sig, 1, 8, f);
  std::vector<uint8_t> ihdr;
  be32(ihdr, (uint32_t)w);
  be32(ihdr, (uint32_t)h);
  ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});  // 8-bit RGB
  chunk(f, "IHDR", ihdr);
  chunk(f, "IDAT", z);
  chunk(f, "IEND", {});
  return std::fclose(f) == 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <scene_dir> <file.cli> [-w W] [-h H] [-spp N] [-seed S] [-device D] "
                         "[-o out.png] [-rgb out.f32] [-tex name=path.ppm]... [-time ITERS] [-nodir] [-budget MS] "
                         "[-noise E [-max N]] [-denoise [LEVELS]] [-eye X Y Z -at X Y Z [-up X Y Z]]\n", argv[0]);
    return 2;
  }
  std::string dir = argv[1], cli = argv[2], out, rgbOut;
  bool inDir = true;
  int W = 300, H = 300, spp = 0, device = 0, timeIters = 0;  // DistRayTracer.java:15-16 default size
  double budgetMs = -1;  // >= 0: accumulate for that long instead of rendering spp samples
  double noise = -1;     // >= 0: sample adaptively down to that standard error
  int maxSamples = 1024;
  bool denoise = false;
  int denoiseLevels = -1;  // >= 0: that many levels instead of the default
  bool haveEye = false, haveAt = false;
  double eye[3] = {0, 0, 0}, at[3] = {0, 0, -1}, up[3] = {0, 1, 0};
  uint64_t seed = 0x5EED0001ull;
  std::vector<std::string> texNames, texPaths;
  for (int i = 3; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); }
      return argv[++i];
    };
    if (a == "-w") W = std::atoi(next().c_str());
    else if (a == "-h") H = std::atoi(next().c_str());
    else if (a == "-spp") spp = std::atoi(next().c_str());
    else if (a == "-seed") seed = std::strtoull(next().c_str(), nullptr, 0);
    else if (a == "-device") device = std::atoi(next().c_str());
    else if (a == "-o") out = next();
    else if (a == "-rgb") rgbOut = next();
    else if (a == "-time") timeIters = std::atoi(next().c_str());
    else if (a == "-nodir") inDir = false;
    else if (a == "-budget") budgetMs = std::atof(next().c_str());
    else if (a == "-noise") noise = std::atof(next().c_str());
    else if (a == "-max") maxSamples = std::atoi(next().c_str());
    else if (a == "-denoise") {
      denoise = true;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') denoiseLevels = std::atoi(argv[++i]);
    }
    else if (a == "-eye") { haveEye = true; for (double& v : eye) v = std::atof(next().c_str()); }
    else if (a == "-at") { haveAt = true; for (double& v : at) v = std::atof(next().c_str()); }
    else if (a == "-up") { for (double& v : up) v = std::atof(next().c_str()); }
    else if (a == "-tex") {
      std::string t = next();
      size_t eq = t.find('=');
      if (eq == std::string::npos) { std::fprintf(stderr, "-tex expects name=path.ppm\n"); return 2; }
      texNames.push_back(t.substr(0, eq));
      texPaths.push_back(t.substr(eq + 1));
    } else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
  }
  double pose[16];
  if (haveEye != haveAt) { std::fprintf(stderr, "-eye and -at go together\n"); return 2; }
  if (haveEye && rt_camera_look_at(eye, at, up, pose)) { std::fprintf(stderr, "%s\n", rt_last_error()); return 2; }
  if (haveEye && noise < 0 && budgetMs < 0 && spp < 1) { std::fprintf(stderr, "-eye expects -spp of at least 1, -budget or -noise\n"); return 2; }
  std::vector<std::vector<uint8_t>> texData(texNames.size());
  std::vector<rt_texture_desc> tex(texNames.size());
  std::vector<const char*> names(texNames.size());
  for (size_t t = 0; t < texNames.size(); ++t) {
    int w = 0, h = 0;
    if (!read_ppm(texPaths[t], w, h, texData[t])) { std::fprintf(stderr, "cannot read %s\n", texPaths[t].c_str()); return 1; }
    tex[t].w = w; tex[t].h = h; tex[t].rgb = texData[t].data();
    names[t] = texNames[t].c_str();
  }
  rt_scene* s = nullptr;
  int rc = rt_scene_load_cli(dir.c_str(), cli.c_str(), (int)tex.size(), names.data(), tex.data(), device, &s);
  if (rc) { std::fprintf(stderr, "rt_scene_load_cli: %d %s\n", rc, rt_last_error()); return 1; }
  if (out.empty()) {
    char name[4096];
    int n = rt_scene_save_name(s, name, (int)sizeof(name));
    if (n < 0 || n >= (int)sizeof(name)) { std::fprintf(stderr, "rt_scene_save_name: %s\n", rt_last_error()); return 1; }
    out = name;
    if (inDir) {
      std::time_t now = std::time(nullptr);
      std::tm tm = *std::localtime(&now);
      char folder[64];  // Calendar.HOUR: 12-hour clock, 0-11
      std::snprintf(folder, sizeof(folder), "pics.%d.%02d.%02d.%02d.%02d", tm.tm_year + 1900, tm.tm_mon + 1, tm.tm_mday,
                    tm.tm_hour % 12, tm.tm_min);
      mkdir(folder, 0755);
      out = std::string(folder) + "/" + out;
    }
  }
  rt_render_params p;
  std::memset(&p, 0, sizeof(p));
  p.width = W; p.height = H; p.spp = spp; p.row0 = 0; p.row1 = H; p.row_step = 1; p.seed = seed;
  std::vector<float> rgb((size_t)W * H * 3);
  std::vector<int32_t> argb((size_t)W * H);
  // the frame of an accumulator: resolved, or with -denoise the denoised one
  auto frame = [&](rt_accum* acc) -> int {
    if (!denoise) return rt_accum_resolve(acc, rgb.data(), argb.data());
    rt_denoise* dn = nullptr;
    rt_denoise_params dp;
    int r = rt_denoise_defaults(&dp);
    if (denoiseLevels >= 0) dp.levels = denoiseLevels;
    if (r == 0) r = rt_denoise_create(acc, &dn);
    if (r == 0) r = rt_denoise_run(dn, &dp, rgb.data(), argb.data());
    rt_denoise_destroy(dn);
    return r;
  };
  // the accumulator of a mode, looking through -eye's pose if one was given
  auto accumulator = [&](uint32_t flags, rt_accum** acc) -> int {
    int r = rt_accum_create(s, &p, flags, acc);
    if (r == 0 && haveEye) r = rt_accum_set_camera(*acc, pose);
    return r;
  };
  if (denoise && noise < 0 && budgetMs < 0 && spp < 2) {
    std::fprintf(stderr, "-denoise expects -spp of at least 2, -budget or -noise\n");
    rt_scene_destroy(s);
    return 2;
  }
  if (noise >= 0) {
    if (maxSamples < 1) { std::fprintf(stderr, "-max expects at least 1\n"); rt_scene_destroy(s); return 2; }
    rt_accum* acc = nullptr;
    rc = accumulator(RT_ACCUM_MOMENTS | RT_ACCUM_COUNTS, &acc);
    int top = maxSamples < 4 ? maxSamples : 4;  // no pixel has more samples than this
    if (rc == 0) rc = rt_accum_add(acc, top, nullptr);
    for (int chunk = 4; rc == 0; chunk = chunk < 64 ? chunk * 2 : 64) {
      int64_t picked = 0;
      rc = rt_accum_select_error(acc, (float)noise, maxSamples, &picked);
      const int c = chunk < maxSamples - top ? chunk : maxSamples - top;
      if (rc || picked == 0 || c < 1) break;
      rc = rt_accum_add_selected(acc, c, nullptr);
      top += c;
    }
    std::vector<int32_t> cnt((size_t)W * H);
    if (rc == 0) rc = rt_accum_counts(acc, cnt.data());
    if (rc == 0) rc = frame(acc);
    rt_accum_destroy(acc);
    if (rc) { std::fprintf(stderr, "rt_accum: %d %s\n", rc, rt_last_error()); rt_scene_destroy(s); return 1; }
    long long total = 0;
    int most = 0;
    for (int32_t v : cnt) { total += v; most = v > most ? v : most; }
    std::printf("pixels %lld samples %lld max %d\n", (long long)W * H, total, most);
  } else if (budgetMs >= 0) {
    rt_accum* acc = nullptr;
    rc = accumulator(denoise ? RT_ACCUM_MOMENTS : 0, &acc);
    int64_t n = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int chunk = 2, first = 1; rc == 0; first = 0) {
      rc = rt_accum_add(acc, chunk, nullptr);
      if (rc == 0) rc = rt_accum_state(acc, &n, nullptr, nullptr);  // waits for the chunk
      if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > budgetMs) break;
      if (!first && chunk < 64) chunk *= 2;  // 2, 2, 4, 8, ... 64, 64, ...
    }
    if (rc == 0) rc = frame(acc);
    rt_accum_destroy(acc);
    if (rc) { std::fprintf(stderr, "rt_accum: %d %s\n", rc, rt_last_error()); rt_scene_destroy(s); return 1; }
    std::printf("samples %lld\n", (long long)n);
  } else if (denoise || haveEye) {
    rt_accum* acc = nullptr;
    rc = accumulator(denoise ? RT_ACCUM_MOMENTS : 0, &acc);
    if (rc == 0) rc = rt_accum_add(acc, spp, nullptr);
    if (rc == 0) rc = frame(acc);
    rt_accum_destroy(acc);
    if (rc) { std::fprintf(stderr, "rt_accum: %d %s\n", rc, rt_last_error()); rt_scene_destroy(s); return 1; }
  } else {
    rc = rt_render(s, &p, rgb.data(), argb.data());
    if (rc) { std::fprintf(stderr, "rt_render: %d %s\n", rc, rt_last_error()); rt_scene_destroy(s); return 1; }
  }
  if (timeIters > 0) {
    double ms = 0;
    rc = rt_time_render(s, &p, 1, timeIters, &ms);
    if (rc == 0) std::printf("render %dx%d: %.3f ms/frame (kernel, %d iters)\n", W, H, ms, timeIters);
  }
  rt_scene_destroy(s);
  if (!write_png(out, W, H, argb.data())) { std::fprintf(stderr, "cannot write %s\n", out.c_str()); return 1; }
  if (!rgbOut.empty()) {
    FILE* f = std::fopen(rgbOut.c_str(), "wb");
    if (!f || std::fwrite(rgb.data(), sizeof(float), rgb.size(), f) != rgb.size()) return 1;
    std::fclose(f);
  }
  std::printf("wrote %s (%dx%d)\n", out.c_str(), W, H);
  return 0;
}
