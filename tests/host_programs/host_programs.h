// host_programs.h — what the stand-alone programs share: a failure count, files in a scratch directory, a 64-bit generator, zlib's
// reading of a gzip file.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <string>
#include <vector>

namespace hp {
struct rng64 {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ULL); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
    uint64_t below(uint64_t n) { return n ? next() % n : 0; }
};
inline int& failures() { static int n = 0; return n; }
inline void fail(const std::string& what) { printf("FAILED %s\n", what.c_str()); fflush(stdout); ++failures(); }
inline int finish() { printf("%s\n", failures() ? "FAILED" : "ok"); return failures() ? 1 : 0; }

inline bool read_file(const std::string& path, std::string& out) {
    out.clear();
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[1 << 16];
    for (size_t r; (r = fread(buf, 1, sizeof buf, f)) > 0;) out.append(buf, r);
    fclose(f);
    return true;
}
inline void write_file(const std::string& path, const std::string& bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || (bytes.size() && fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
}
// a fresh directory for the run's files: the destructor removes the files and sub-directories that were asked for, then the directory
struct scratch_dir {
    std::string path; std::vector<std::string> files, dirs;
    scratch_dir() { char t[] = "/tmp/vg_host_XXXXXX"; if (!mkdtemp(t)) { perror("mkdtemp"); exit(2); } path = t; }
    std::string file(const std::string& name) { files.push_back(path + "/" + name); return files.back(); }
    std::string dir(const std::string& name) { dirs.push_back(path + "/" + name); if (mkdir(dirs.back().c_str(), 0700) != 0) { perror("mkdir"); exit(2); } return dirs.back(); }
    ~scratch_dir() { for (const std::string& f : files) unlink(f.c_str()); for (const std::string& d : dirs) rmdir(d.c_str()); rmdir(path.c_str()); }
};
// FNV-1a over bytes: arrays and files are reported by length and this
inline uint64_t fnv(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ULL) {
    for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)p)[i]; h *= 0x100000001b3ULL; }
    return h;
}
// what zlib's gzip reader makes of the bytes: members one after the other; zeros, or anything that is no gzip magic, behind a
// complete member are ignored; false = an error (a damaged or cut member)
inline bool zlib_gunzip(const unsigned char* in, size_t n, std::string& out) {
    out.clear();
    size_t at = 0; bool any = false;
    while (at < n) {
        if (any) {
            while (at < n && in[at] == 0) ++at;
            if (at == n) break;
            if (n - at < 2 || in[at] != 0x1f || in[at + 1] != 0x8b) break;      // trailing garbage
        }
        z_stream zs; memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
        zs.next_in = (Bytef*)in + at; zs.avail_in = (uInt)(n - at);
        int rc = Z_OK;
        while (rc == Z_OK) {
            const size_t have = out.size(); out.resize(have + (1u << 20));
            zs.next_out = (Bytef*)&out[have]; zs.avail_out = 1u << 20;
            rc = inflate(&zs, Z_NO_FLUSH);
            out.resize(have + ((1u << 20) - zs.avail_out));
            if (rc == Z_OK && zs.avail_in == 0 && zs.avail_out != 0) rc = Z_BUF_ERROR;      // the input ended inside the member
        }
        at = n - zs.avail_in;
        inflateEnd(&zs);
        if (rc != Z_STREAM_END) return false;
        any = true;
    }
    return any;
}
}  // namespace hp
