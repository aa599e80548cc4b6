// Activation arena of the network executor (net_build.hip): the first-fit offset planner and the tensor record that knows whether it owns
// its block.  Standard C++ only (no HIP include): tests/arena_check.cpp builds this header with the host compiler.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <vector>

#ifdef __FLT16_MANT_DIG__
typedef _Float16 f16;
#else
typedef unsigned short f16;   // a host compiler without _Float16: the arena only steps pointers over the two bytes
#endif

namespace sdeo {

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Arena {   // first-fit planner over one device allocation; offsets only
  struct Blk_ { size_t off, size; bool free; };
  std::vector<Blk_> blocks;
  size_t end = 0, peak = 0;
  size_t alloc(size_t bytes) {
    bytes = align_up(bytes, 256);
    for (size_t i = 0; i < blocks.size(); ++i) {
      if (blocks[i].free && blocks[i].size >= bytes) {
        if (blocks[i].size > bytes) {
          Blk_ rest{blocks[i].off + bytes, blocks[i].size - bytes, true};
          blocks[i].size = bytes;
          blocks.insert(blocks.begin() + i + 1, rest);
        }
        blocks[i].free = false;
        return blocks[i].off;
      }
    }
    if (!blocks.empty() && blocks.back().free) {   // grow the trailing free block
      blocks.back().size = bytes;
      blocks.back().free = false;
      end = blocks.back().off + bytes;
      peak = std::max(peak, end);
      return blocks.back().off;
    }
    blocks.push_back({end, bytes, false});
    end += bytes;
    peak = std::max(peak, end);
    return blocks.back().off;
  }
  void release(size_t off) {
    for (size_t i = 0; i < blocks.size(); ++i) {
      if (blocks[i].off == off && !blocks[i].free) {
        blocks[i].free = true;
        if (i + 1 < blocks.size() && blocks[i + 1].free) { blocks[i].size += blocks[i + 1].size; blocks.erase(blocks.begin() + i + 1); }
        if (i > 0 && blocks[i - 1].free) { blocks[i - 1].size += blocks[i].size; blocks.erase(blocks.begin() + i); }
        return;
      }
    }
  }
};

struct T {           // fp16 activation view: rows x c, row stride ld; (n,h,w) when it is an image
  static constexpr size_t kNone = (size_t)-1;   // "no arena block": a view of someone else's tensor / no GroupNorm partials
  f16* p = nullptr;
  size_t off = kNone;        // arena offset when owned
  int n = 0, h = 0, w = 0, c = 0, ld = 0;
  // GroupNorm partials of this tensor written by the epilogue of the conv / GEMM that produced it (ConvGemm::gn_out), 32 groups
  float* gnp = nullptr;
  size_t gnp_off = kNone;    // reserved arena block of the partials (gnp stays null when the plan cannot emit them)
  int gn_slots = 0;
  int rows() const { return n * h * w; }
  bool owned() const { return off != kNone; }
  bool gn_reserved() const { return gnp_off != kNone; }
  // columns [col0, col0 + cols) of every row: same image, same row stride; releasing it releases nothing
  T view(int col0, int cols) const {
    T v;
    v.p = p + col0; v.n = n; v.h = h; v.w = w; v.c = cols; v.ld = ld;
    return v;
  }
  T view() const { return view(0, c); }
  // give the blocks back (nothing for a view); what is left is a view of memory that may be handed out again
  void release(Arena& a) {
    if (owned()) a.release(off);
    if (gn_reserved()) a.release(gnp_off);
    off = gnp_off = kNone;
    gnp = nullptr;
  }
};

}  // namespace sdeo
