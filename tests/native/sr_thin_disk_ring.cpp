// sr::ThinDisk's f64 capture band through the C++ host mirror
// (include/geo/sr.hpp): one small frame of the sky sphere with its thin disk,
// plain, with the band in f64 (set_ring_f64) and plain again
// (set_ring_f64(false)); FNV-1a of each.  tests/test_cpp_thin_disk_ring.py
// compares them with the CPU path's frames (geo_render_cpu_disk_ring_f64).
//
// The scene is the third image's: an observer at rest at (14, 0, 5.1), a
// narrow camera (fov 0.004) raised by THETA onto the photon ring's edge, the
// disk 3..9 (tests/test_disk_cpu.py's pose "ring").
//
//   sr_thin_disk_ring W H THETA
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "geo/sr.hpp"

namespace {

uint64_t fnv1a(const std::vector<uint8_t>& b) {
    uint64_t h = 1469598103934665603ull;
    for (uint8_t x : b) h = (h ^ x) * 1099511628211ull;
    return h;
}

// sr_reference_tests.cpp's synthetic texture at any size
sr::Image pattern(uint32_t w, uint32_t h) {
    sr::Image im;
    im.width = w;
    im.height = h;
    im.rgba.resize((size_t)w * h * 4);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            uint8_t* t = &im.rgba[4 * ((size_t)y * w + x)];
            t[0] = (uint8_t)((x * 7u) ^ (y * 13u));
            t[1] = (uint8_t)(x + y);
            t[2] = (uint8_t)(x * y);
            t[3] = 255;
        }
    return im;
}

uint64_t draw(sr::Renderer& renderer, sr::BasicSphereBuffer& sky, const sr::ThinDisk& disk) {
    sky.set_thin_disk(disk);
    renderer.render({&sky}, {});
    return fnv1a(renderer.read_frame());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s W H THETA\n", argv[0]);
        return 2;
    }
    try {
        sr::Renderer renderer((uint32_t)std::atoi(argv[1]), (uint32_t)std::atoi(argv[2]), 1.0, 0.004);
        renderer.observer().set_position({14.0, 0.0, 5.1});
        renderer.observer().set_camera(sr::kPi, std::strtod(argv[3], nullptr));
        renderer.observer().start_unmoving();
        sr::BasicSphereBuffer sky(0, 50.0, 1.0, pattern(512, 256), GEO_MODE_DIRECT, 2048);
        sky.update_ray_fan(renderer.get_radial_position());
        sr::ThinDisk disk;
        disk.texture = pattern(64, 16);
        disk.r_in = 3.0f;
        disk.r_out = 9.0f;
        const uint64_t plain = draw(renderer, sky, disk);
        const uint64_t ring = draw(renderer, sky, disk.set_ring_f64());
        const uint64_t off = draw(renderer, sky, disk.set_ring_f64(false));
        std::printf("disk fnv1a %016llx\ndisk+ring fnv1a %016llx\ndisk off fnv1a %016llx\n", (unsigned long long)plain,
                    (unsigned long long)ring, (unsigned long long)off);
        return 0;
    } catch (const sr::Error& e) {
        std::fprintf(stderr, "sr::Error: %s\n", e.what());
        return 3;
    }
}
