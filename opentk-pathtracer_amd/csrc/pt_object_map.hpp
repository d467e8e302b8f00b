// pt_object_map.hpp — the object map of the temporal stage's object tracking (pt_denoise_set_object_tracking): the
// host's comparison of the scene a history set was made of with the scene in force.  Plain C++ without HIP, so that a host-only program
// can include it (tests/test_tracking_object_map_host.py compares it with the numpy restatement, degenerate geometry included).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>

namespace ptmap {

constexpr int kMaxSpheres = 256, kMaxCuboids = 64; // PT_MAX_SPHERES, PT_MAX_CUBOIDS
constexpr int kEntries = kMaxSpheres + kMaxCuboids, kEntryBytes = 32;
constexpr int kKeep = 0, kMoved = 1, kDrop = 2;    // PT_TRACK_KEEP, PT_TRACK_MOVED, PT_TRACK_DROP

// Per guide id k (sphere i at i, cuboid j at kMaxSpheres + j) 8 words into map — a.xyz, state, b.xyz, 0 — from the history's scene blob and
// counts (histScene, histSpheres, histCuboids) against those in force (scene, ns, nc).
// DROP: k is beyond either scene's count of its kind, or its 64 material bytes differ; KEEP (a = 1, b = 0): its geometry floats (sphere:
// centre and radius; cuboid: min and max, the std140 pad words not compared) are bit-equal; else MOVED with the map history = a * current
// + b that carries the current object onto the history's — sphere: a = r_h / r_c on all axes, cuboid: a = extent_h / extent_c per axis,
// b = (c_h | min_h) - a * (c_c | min_c) — formed in double from the binary32 fields and rounded once, where both radii / every extent are
// > 0 and everything is finite, else DROP (a = b = 0).  -> the tracked kernel has to run (an id that exists is not KEEP, or the counts differ).
inline bool build(const unsigned char *histScene, int histSpheres, int histCuboids, const unsigned char *scene, int ns, int nc, unsigned char *map)
{
    bool tracked = histSpheres != ns || histCuboids != nc;
    for (int k = 0; k < kEntries; k++) {
        const bool sphere = k < kMaxSpheres;
        const int i = sphere ? k : k - kMaxSpheres;
        const size_t at = sphere ? (size_t)80 * i : (size_t)kMaxSpheres * 80 + (size_t)96 * i, geo = sphere ? 16 : 32;
        const bool exists = sphere ? i < histSpheres && i < ns : i < histCuboids && i < nc;
        float a[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
        int state = kDrop;
        if (exists && std::memcmp(histScene + at + geo, scene + at + geo, 64) == 0) {
            float gh[8], gc[8];
            std::memcpy(gh, histScene + at, geo);
            std::memcpy(gc, scene + at, geo);
            const bool same = sphere ? std::memcmp(gh, gc, 16) == 0 : std::memcmp(gh, gc, 12) == 0 && std::memcmp(gh + 4, gc + 4, 12) == 0;
            if (same) {
                state = kKeep;
                a[0] = a[1] = a[2] = 1.0f;
            } else {
                bool ok = true;
                for (int c = 0; c < 3; c++) {
                    const double eh = sphere ? (double)gh[3] : (double)gh[4 + c] - (double)gh[c];
                    const double ec = sphere ? (double)gc[3] : (double)gc[4 + c] - (double)gc[c];
                    // (the order matters: the quotient is only formed, and only rounded to binary32, where it is defined and finite)
                    if (!(eh > 0.0 && ec > 0.0 && std::isfinite(eh) && std::isfinite(ec) && std::isfinite(gh[c]) && std::isfinite(gc[c]))) {
                        ok = false;
                        break;
                    }
                    const double q = eh / ec, off = (double)gh[c] - q * (double)gc[c];
                    if (!(std::fabs(q) < 0x1.ffffffp127 && std::fabs(off) < 0x1.ffffffp127)) { // (rounds to a finite binary32: below FLT_MAX + half an ulp)
                        ok = false;
                        break;
                    }
                    a[c] = (float)q;
                    b[c] = (float)off;
                }
                if (ok) {
                    state = kMoved;
                } else {
                    a[0] = a[1] = a[2] = b[0] = b[1] = b[2] = 0.0f;
                }
            }
        }
        if (exists && state != kKeep) tracked = true;
        unsigned char *e = map + (size_t)kEntryBytes * k;
        std::memset(e, 0, kEntryBytes);
        std::memcpy(e, a, 12);
        std::memcpy(e + 12, &state, 4);
        std::memcpy(e + 16, b, 12);
    }
    return tracked;
}

} // namespace ptmap
