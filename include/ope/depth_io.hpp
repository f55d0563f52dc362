// depth_io.hpp — the sensor's depth image on the host and its file form, for programs that read recorded frames.
// DepthImage stands where the reference has a cv::Mat of CV_16UC1 (rosinterface.cpp:407-422): rows, cols, a row step in bytes
// and the samples.  loadPGM reads a binary PGM ("P5", maxval <= 65535; two bytes per sample, most significant first, when
// maxval > 255) in the style of pcd_io.hpp: 0, or -1 with one line on stderr and the image left empty.  savePGM writes one.
#pragma once

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

namespace ope {

struct DepthImage {
  size_t rows = 0, cols = 0;
  size_t step = 0;                 // bytes from one row to the next (cv::Mat::step), >= 2 * cols and even
  std::vector<uint16_t> data;      // rows * step / 2 samples
  DepthImage() {}
  DepthImage(size_t r, size_t c) : rows(r), cols(c), step(2 * c), data(r * c, 0) {}
  uint16_t &at(size_t r, size_t c) { return data[r * (step / 2) + c]; }          // p_imageDepth.at<unsigned short>(i, j)
  const uint16_t &at(size_t r, size_t c) const { return data[r * (step / 2) + c]; }
  bool empty() const { return rows == 0 || cols == 0; }
};

namespace io {

inline int loadPGM(const std::string &file_name, DepthImage &image) {
  image = DepthImage();
  auto fail = [&](const char *what) {
    std::fprintf(stderr, "[ope::io::loadPGM] '%s': %s.\n", file_name.c_str(), what);
    image = DepthImage();
    return -1;
  };
  std::ifstream f(file_name, std::ios::binary);
  if (!f) { std::fprintf(stderr, "[ope::io::loadPGM] Could not find file '%s'.\n", file_name.c_str()); return -1; }
  char magic[2] = {0, 0};
  f.read(magic, 2);
  if (f.gcount() != 2 || magic[0] != 'P' || magic[1] != '5') return fail("not a binary PGM (P5)");
  long vals[3] = {0, 0, 0};
  for (int k = 0; k < 3; ++k) {
    // white space and comments in front of the number; at least one separator
    int c = f.get(), skipped = 0;
    for (;;) {
      if (c == ' ' || c == '\t' || c == '\r' || c == '\n') { ++skipped; c = f.get(); }
      else if (c == '#' && skipped) { while (c != '\n' && c != EOF) c = f.get(); }
      else break;
    }
    if (!skipped || c < '0' || c > '9') return fail("malformed header");
    long v = 0;
    int digits = 0;
    while (c >= '0' && c <= '9') { v = v * 10 + (c - '0'); if (++digits > 9) return fail("malformed header"); c = f.get(); }
    vals[k] = v;
    if (k < 2) f.unget();
    else if (!(c == ' ' || c == '\t' || c == '\r' || c == '\n')) return fail("no separator after maxval");
  }
  const long cols = vals[0], rows = vals[1], maxval = vals[2];
  if (cols < 1 || rows < 1 || maxval < 1 || maxval > 65535) return fail("bad size or maxval");
  if ((unsigned long long)rows * (unsigned long long)cols > 0x7fffffffull) return fail("more than 2^31 - 1 pixels");
  const size_t width = maxval < 256 ? 1 : 2, n = (size_t)rows * (size_t)cols;
  std::vector<unsigned char> buf;
  try { buf.resize(n * width); image.data.resize(n); } catch (const std::exception &) { return fail("out of memory"); }
  f.read(reinterpret_cast<char *>(buf.data()), (std::streamsize)buf.size());
  if ((size_t)f.gcount() != buf.size()) return fail("file shorter than its header says");
  for (size_t i = 0; i < n; ++i)
    image.data[i] = width == 2 ? (uint16_t)((buf[2 * i] << 8) | buf[2 * i + 1]) : (uint16_t)buf[i];
  image.rows = (size_t)rows;
  image.cols = (size_t)cols;
  image.step = 2 * (size_t)cols;
  return 0;
}

inline int savePGM(const std::string &file_name, const DepthImage &image) {
  std::ofstream f(file_name, std::ios::binary);
  if (!f) { std::fprintf(stderr, "[ope::io::savePGM] Could not open '%s' for writing.\n", file_name.c_str()); return -1; }
  f << "P5\n" << image.cols << " " << image.rows << "\n65535\n";
  for (size_t r = 0; r < image.rows; ++r)
    for (size_t c = 0; c < image.cols; ++c) {
      const uint16_t v = image.at(r, c);
      const char be[2] = {(char)(v >> 8), (char)(v & 0xff)};
      f.write(be, 2);
    }
  return f ? 0 : -1;
}

}  // namespace io
}  // namespace ope
