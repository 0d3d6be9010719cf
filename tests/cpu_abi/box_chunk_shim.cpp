// C entry point over csrc/bq_box_chunk.h for tests/test_host_entry_points_cpu.py: walks a box list the way the launcher of
// fl_box_pack / fl_box_unpack / fl_box_copy does and records every chunk.  Test infrastructure.
#include "bq_box_chunk.h"

namespace {
struct Box { int x0, x1, y0, y1, z0, z1; };     // layout of fl_box (include/bimocq_gpu.h)
}

extern "C" {

int box_chunk_limit(void) { return bq::box::kBoxChunk; }

// boxes: nboxes rows of (x0, x1, y0, y1, z0, z1).  Per chunk: ranges gets (first, next, n, packed elements); per slot of a
// chunk: slots gets (x0, y0, z0, wx, wy, offset inside the chunk).  Returns the number of chunks, -1 when one of the
// output arrays (max_chunks / max_slots rows) is too small -- which also ends a walk that does not advance.
int box_chunk_walk(const int *boxes, int nboxes, long long *ranges, int max_chunks, long long *slots, int max_slots)
{
    const Box *list = reinterpret_cast<const Box *>(boxes);
    int chunks = 0, used = 0;
    for (int first = 0; first < nboxes;) {
        bq::box::BoxChunk c;
        const int next = bq::box::fill_chunk(list, nboxes, first, c);
        if (chunks >= max_chunks || used + c.n > max_slots || next <= first) return -1;
        long long *r = ranges + 4 * chunks++;
        r[0] = first; r[1] = next; r[2] = c.n; r[3] = c.off[c.n];
        for (int s = 0; s < c.n; s++) {
            long long *q = slots + 6 * used++;
            q[0] = c.x0[s]; q[1] = c.y0[s]; q[2] = c.z0[s]; q[3] = c.wx[s]; q[4] = c.wy[s]; q[5] = c.off[s];
        }
        first = next;
    }
    return chunks;
}

} // extern "C"
