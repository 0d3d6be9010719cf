// bq_box_chunk.h -- how fl_box_pack / fl_box_unpack / fl_box_copy (bq_halo.hip) cut a box list into kernel launches.  A launch
// takes its boxes by value, kBoxChunk at most; zero-volume boxes take no slot.  Pure host code: no HIP, no runtime state, so
// that tests/test_host_entry_points_cpu.py can compile it with a plain C++ compiler and check the rule without a GPU.
#pragma once

namespace bq {
namespace box {

constexpr int kBoxChunk = 64;
struct BoxChunk {
    int n;
    int x0[kBoxChunk], y0[kBoxChunk], z0[kBoxChunk], wx[kBoxChunk], wy[kBoxChunk];
    long long off[kBoxChunk + 1];       // element offset of each box inside this chunk's packed range
};

// Fills `c` with the non-empty boxes of boxes[first .. nboxes) in order until it holds kBoxChunk of them or the list ends, and
// returns the index of the first box it did NOT consume: where the next chunk starts.  Every box is so consumed exactly once,
// and the chunks' packed ranges follow each other without gap or overlap.  Box: half-open x0, x1, y0, y1, z0, z1 (fl_box), valid.
template <class Box>
inline int fill_chunk(const Box *boxes, int nboxes, int first, BoxChunk &c)
{
    c.n = 0; c.off[0] = 0;
    int b = first;
    for (; b < nboxes && c.n < kBoxChunk; b++) {
        const Box &q = boxes[b];
        const long long vol = (long long)(q.x1 - q.x0) * (q.y1 - q.y0) * (q.z1 - q.z0);
        if (vol == 0) continue;
        c.x0[c.n] = q.x0; c.y0[c.n] = q.y0; c.z0[c.n] = q.z0; c.wx[c.n] = q.x1 - q.x0; c.wy[c.n] = q.y1 - q.y0;
        c.off[c.n + 1] = c.off[c.n] + vol;
        c.n++;
    }
    return b;
}

} // namespace box
} // namespace bq
