// The ranks of a mesh as THREADS of one process on one GPU: ghost rows and packed ghost columns through an in-process
// mailbox with the contract of ststhip_comm_exchange_rows (RCCL cannot join several ranks on one device).  Used by
// block_template_test (tests/cpp) and by the mesh mode of shape_test_a ... shape_test_d (tests/cpp_shapes); strips of n
// ranks are a mesh of n x 1 with the row exchange alone.
//
// Every wait is bounded: a mesh whose ranks disagree (one plans another exchange than its neighbour, or has failed)
// ends the process with a distinct exit status, after naming the rank, the edge and the bytes, and never hangs.
#pragma once
#include <ststhip.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

namespace mesh_harness {

constexpr int exit_call_failed = 2, exit_wait_expired = 3, exit_size_mismatch = 4;

#define MESH_CHECK(call)                                                                            \
    do {                                                                                            \
        int rc_ = (call);                                                                           \
        if (rc_ != STSTHIP_OK) {                                                                    \
            std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ststhip_last_error());         \
            std::_Exit(mesh_harness::exit_call_failed);                                             \
        }                                                                                           \
    } while (0)

// one directed edge of the mesh: a buffer of one message
struct Edge {
    std::mutex m;
    std::condition_variable cv;
    bool full = false;
    std::vector<std::vector<unsigned char>> planes;
    // for the report of a wait that expired: who sends over this edge and where to
    int sender = -1;
    const char *direction = "?";
    // a step of these tests is a few kernel launches and copies of some kilobytes: milliseconds
    std::chrono::seconds limit{30};

    static std::size_t total(std::vector<std::vector<unsigned char>> const &message) {
        std::size_t bytes = 0;
        for (auto const &plane : message)
            bytes += plane.size();
        return bytes;
    }
    void put(int n_planes, const void *const *device, const size_t *row_bytes, size_t n_rows, ststhip_stream stream) {
        std::vector<std::vector<unsigned char>> message(n_planes);
        for (int p = 0; p < n_planes; p++) {
            message[p].resize(row_bytes[p] * n_rows);
            MESH_CHECK(ststhip_memcpy_d2h(message[p].data(), device[p], message[p].size(), stream));
        }
        MESH_CHECK(ststhip_stream_synchronize(stream));
        std::unique_lock<std::mutex> lock(m);
        if (!cv.wait_for(lock, limit, [&] { return !full; })) {
            std::fprintf(stderr,
                         "mailbox: rank %d, edge %s: the message before this one (%zu bytes) was not taken within %lld s; "
                         "%zu bytes wait to be sent\n",
                         sender, direction, total(planes), static_cast<long long>(limit.count()), total(message));
            std::_Exit(exit_wait_expired);
        }
        planes.swap(message);
        full = true;
        cv.notify_all();
    }
    void take(int receiver, int n_planes, void *const *device, const size_t *row_bytes, size_t n_rows, ststhip_stream stream) {
        std::size_t expected = 0;
        for (int p = 0; p < n_planes; p++)
            expected += row_bytes[p] * n_rows;
        std::vector<std::vector<unsigned char>> message;
        {
            std::unique_lock<std::mutex> lock(m);
            if (!cv.wait_for(lock, limit, [&] { return full; })) {
                std::fprintf(stderr,
                             "mailbox: rank %d, edge %s of rank %d: expected %zu bytes, received nothing within %lld s\n",
                             receiver, direction, sender, expected, static_cast<long long>(limit.count()));
                std::_Exit(exit_wait_expired);
            }
            message.swap(planes);
            full = false;
            cv.notify_all();
        }
        bool fits = int(message.size()) == n_planes;
        for (int p = 0; fits && p < n_planes; p++)
            fits = message[p].size() == row_bytes[p] * n_rows;
        if (!fits) {
            std::fprintf(stderr, "mailbox: rank %d, edge %s of rank %d: expected %zu bytes in %d planes, received %zu in %zu\n",
                         receiver, direction, sender, expected, n_planes, total(message), message.size());
            std::_Exit(exit_size_mismatch);
        }
        for (int p = 0; p < n_planes; p++)
            MESH_CHECK(ststhip_memcpy_h2d(device[p], message[p].data(), message[p].size(), stream));
        MESH_CHECK(ststhip_stream_synchronize(stream));
    }
};
struct Mesh {
    int rows, cols;
    std::vector<Edge> to_up, to_down, to_left, to_right; // indexed by the SENDING rank
    Mesh(int r, int c) : rows(r), cols(c), to_up(r * c), to_down(r * c), to_left(r * c), to_right(r * c) {
        for (int rank = 0; rank < r * c; rank++) {
            to_up[rank].sender = to_down[rank].sender = to_left[rank].sender = to_right[rank].sender = rank;
            to_up[rank].direction = "to_up", to_down[rank].direction = "to_down";
            to_left[rank].direction = "to_left", to_right[rank].direction = "to_right";
        }
    }
};
struct Side {
    Mesh *mesh;
    int rank;
};
// the contract of ststhip_comm_exchange_rows; "first" / "second" neighbour = up / down for rows, left / right for columns
inline int exchange_rows(void *ctx, int n_planes, const void *const *send_up, const void *const *send_down,
                         void *const *recv_up, void *const *recv_down, const size_t *row_bytes, size_t n_rows,
                         ststhip_stream stream) {
    Side *s = static_cast<Side *>(ctx);
    Mesh &m = *s->mesh;
    const int r = s->rank / m.cols;
    MESH_CHECK(ststhip_stream_synchronize(stream));
    if (r > 0)
        m.to_up[s->rank].put(n_planes, send_up, row_bytes, n_rows, stream);
    if (r + 1 < m.rows)
        m.to_down[s->rank].put(n_planes, send_down, row_bytes, n_rows, stream);
    if (r > 0)
        m.to_down[s->rank - m.cols].take(s->rank, n_planes, recv_up, row_bytes, n_rows, stream);
    if (r + 1 < m.rows)
        m.to_up[s->rank + m.cols].take(s->rank, n_planes, recv_down, row_bytes, n_rows, stream);
    return STSTHIP_OK;
}
inline int exchange_cols(void *ctx, int n_planes, const void *const *send_left, const void *const *send_right,
                         void *const *recv_left, void *const *recv_right, const size_t *row_bytes, size_t n_rows,
                         ststhip_stream stream) {
    Side *s = static_cast<Side *>(ctx);
    Mesh &m = *s->mesh;
    const int c = s->rank % m.cols;
    MESH_CHECK(ststhip_stream_synchronize(stream));
    if (c > 0)
        m.to_left[s->rank].put(n_planes, send_left, row_bytes, n_rows, stream);
    if (c + 1 < m.cols)
        m.to_right[s->rank].put(n_planes, send_right, row_bytes, n_rows, stream);
    if (c > 0)
        m.to_right[s->rank - 1].take(s->rank, n_planes, recv_left, row_bytes, n_rows, stream);
    if (c + 1 < m.cols)
        m.to_left[s->rank + 1].take(s->rank, n_planes, recv_right, row_bytes, n_rows, stream);
    return STSTHIP_OK;
}

} // namespace mesh_harness
