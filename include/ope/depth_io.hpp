// depth_io.hpp — the sensor's depth image on the host and its file form, for programs that read recorded frames.
// DepthImage stands where the reference has a cv::Mat of CV_16UC1 (rosinterface.cpp:407-422): rows, cols, a row step in bytes
// and the samples.  loadPGM reads a binary PGM ("P5", maxval <= 65535; two bytes per sample, most significant first, when
// maxval > 255) in the style of pcd_io.hpp: 0, or -1 with one line on stderr and the image left empty.  savePGM writes one.
// ColorImage stands where the reference has a cv::Mat of CV_8UC3 (BuildModel datagrabber.cpp:9): three bytes per pixel in
// OpenCV's order B, G, R.  loadPPM reads the 8-bit counterpart of the PGM, a binary PPM ("P6", maxval <= 255), whose samples
// are R, G, B, and swaps them into that order as cv::imread does; savePPM swaps them back.
#pragma once

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <utility>
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

struct ColorImage {
  size_t rows = 0, cols = 0;
  size_t step = 0;                    // bytes from one row to the next, >= 3 * cols
  std::vector<unsigned char> data;    // rows * step bytes, pixel (r, c) at r * step + 3 * c: b, g, r
  ColorImage() {}
  ColorImage(size_t r, size_t c) : rows(r), cols(c), step(3 * c), data(r * c * 3, 0) {}
  unsigned char *at(size_t r, size_t c) { return data.data() + r * step + 3 * c; }          // p_imageRgb.at<cv::Vec3b>(i, j)
  const unsigned char *at(size_t r, size_t c) const { return data.data() + r * step + 3 * c; }
  bool empty() const { return rows == 0 || cols == 0; }
};

namespace io {

// the three header numbers behind the magic number of a binary PNM file (white space and comments between them, one separator
// behind the last); false: malformed
inline bool readPnmHeader(std::ifstream &f, long vals[3]) {
  for (int k = 0; k < 3; ++k) {
    int c = f.get(), skipped = 0;
    for (;;) {
      if (c == ' ' || c == '\t' || c == '\r' || c == '\n') { ++skipped; c = f.get(); }
      else if (c == '#' && skipped) { while (c != '\n' && c != EOF) c = f.get(); }
      else break;
    }
    if (!skipped || c < '0' || c > '9') return false;
    long v = 0;
    int digits = 0;
    while (c >= '0' && c <= '9') { v = v * 10 + (c - '0'); if (++digits > 9) return false; c = f.get(); }
    vals[k] = v;
    if (k < 2) f.unget();
    else if (!(c == ' ' || c == '\t' || c == '\r' || c == '\n')) return false;
  }
  return true;
}

inline int loadPPM(const std::string &file_name, ColorImage &image) {
  image = ColorImage();
  auto fail = [&](const char *what) {
    std::fprintf(stderr, "[ope::io::loadPPM] '%s': %s.\n", file_name.c_str(), what);
    image = ColorImage();
    return -1;
  };
  std::ifstream f(file_name, std::ios::binary);
  if (!f) { std::fprintf(stderr, "[ope::io::loadPPM] Could not find file '%s'.\n", file_name.c_str()); return -1; }
  char magic[2] = {0, 0};
  f.read(magic, 2);
  if (f.gcount() != 2 || magic[0] != 'P' || magic[1] != '6') return fail("not a binary PPM (P6)");
  long vals[3] = {0, 0, 0};
  if (!readPnmHeader(f, vals)) return fail("malformed header");
  const long cols = vals[0], rows = vals[1], maxval = vals[2];
  if (cols < 1 || rows < 1 || maxval < 1 || maxval > 255) return fail("bad size or maxval (8-bit samples only)");
  if ((unsigned long long)rows * (unsigned long long)cols > 0x7fffffffull) return fail("more than 2^31 - 1 pixels");
  const size_t n = (size_t)rows * (size_t)cols;
  try { image.data.resize(3 * n); } catch (const std::exception &) { return fail("out of memory"); }
  f.read(reinterpret_cast<char *>(image.data.data()), (std::streamsize)image.data.size());
  if ((size_t)f.gcount() != image.data.size()) return fail("file shorter than its header says");
  for (size_t i = 0; i < n; ++i) std::swap(image.data[3 * i], image.data[3 * i + 2]);   // R G B in the file, B G R in memory
  image.rows = (size_t)rows;
  image.cols = (size_t)cols;
  image.step = 3 * (size_t)cols;
  return 0;
}

inline int savePPM(const std::string &file_name, const ColorImage &image) {
  std::ofstream f(file_name, std::ios::binary);
  if (!f) { std::fprintf(stderr, "[ope::io::savePPM] Could not open '%s' for writing.\n", file_name.c_str()); return -1; }
  f << "P6\n" << image.cols << " " << image.rows << "\n255\n";
  for (size_t r = 0; r < image.rows; ++r)
    for (size_t c = 0; c < image.cols; ++c) {
      const unsigned char *p = image.at(r, c);
      const char rgb[3] = {(char)p[2], (char)p[1], (char)p[0]};
      f.write(rgb, 3);
    }
  return f ? 0 : -1;
}

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
