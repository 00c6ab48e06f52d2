// dist_save.h -- one file written by all ranks (dist_text.hip: the FASTA file; dist_gfa.hip: the GFA file): rank 0 creates it at
// its full length, every rank copies its parts of the text down a chunk at a time and writes them at their offsets, write errors are
// agreed at the end, and a call that fails after the file was created leaves none behind.  For ranks that are threads of one process
// and for process ranks that see one filesystem.  KATOME_DIST_TEXT_CHUNK=<bytes>: the host buffer (default 64 MiB).
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "dist_agree.h"

namespace katome {

struct FilePart { const uint8_t* d_bytes; uint64_t n, at; };      // device bytes of this rank and where they start in the file

// all of `buf` at `at`, whatever pwrite makes of it in one go
inline int write_at(int fd, const uint8_t* buf, uint64_t n, uint64_t at, const char* path) {
    while (n) {
        const ssize_t w = pwrite(fd, buf, n, (off_t)at);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) { set_error("couldn't write %s: %s", path, strerror(errno)); return KATOME_E_OPEN; }
        buf += w; n -= (uint64_t)w; at += (uint64_t)w;
    }
    return KATOME_OK;
}

// collective: `total` bytes in all, this rank's `parts` among them
inline int save_parts(katome_comm* comm, const char* name, const char* path, uint64_t total, const FilePart* parts, int n_parts, hipStream_t stream) {
    Collective C(comm, name);
    const bool root = C.rank == 0;
    int fd = -1;
    bool created = false;
    // rank 0 makes the file at its full length; why it could not travels as a number, so every rank reports the reference's message
    uint64_t why = 0;
    if (root) {
        fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) why = create_error_kind(errno);
        else {
            created = true;
            if (ftruncate(fd, (off_t)total) != 0) why = create_error_kind(errno);
        }
    }
    auto finish = [&](int rc) -> int {
        if (fd >= 0 && close(fd) != 0 && !rc) { set_error("couldn't write %s: %s", path, strerror(errno)); rc = KATOME_E_OPEN; }
        fd = -1;
        return rc;
    };
    auto failed = [&](int rc) -> int {                       // (a caller never finds a partial file)
        const std::string keep = get_error();
        finish(rc);
        if (created) (void)unlink(path);
        set_error("%s", keep.c_str());
        return rc;
    };
    { const int rc = C.agree(KATOME_OK, &why); if (rc) return failed(rc); }
    if (why) { set_error("couldn't create %s: %s", path, CREATE_ERROR_KINDS[why < 5 ? why : 4]); return failed(KATOME_E_OPEN); }      // asm/mod.rs:62
    auto copy_out = [&]() -> int {
        uint64_t largest = 0;
        for (int q = 0; q < n_parts; ++q) largest = std::max(largest, parts[q].n);
        if (largest == 0) return KATOME_OK;
        if (!root) {
            fd = open(path, O_WRONLY);
            if (fd < 0) { set_error("couldn't open %s to write this rank's part: %s", path, strerror(errno)); return KATOME_E_OPEN; }
        }
        uint64_t chunk = 64ull << 20;
        if (const char* e = getenv("KATOME_DIST_TEXT_CHUNK")) chunk = std::max<long long>(1, atoll(e));
        chunk = std::min(chunk, largest);
        std::vector<uint8_t> buf;
        try { buf.resize(chunk); }
        catch (const std::bad_alloc&) { set_error("out of host memory"); return KATOME_E_OOM; }
        for (int q = 0; q < n_parts; ++q)
            for (uint64_t at = 0; at < parts[q].n; at += chunk) {
                const uint64_t cnt = std::min(chunk, parts[q].n - at);
                KCHECK_HIP(hipMemcpyAsync(buf.data(), parts[q].d_bytes + at, cnt, hipMemcpyDeviceToHost, stream));
                KCHECK_HIP(hipStreamSynchronize(stream));
                KCHECK(write_at(fd, buf.data(), cnt, parts[q].at + at, path));
            }
        return KATOME_OK;
    };
    const int rc = C.agree(finish(copy_out()));              // (the closing agreement carries the write errors)
    return rc ? failed(rc) : KATOME_OK;
}

}  // namespace katome
