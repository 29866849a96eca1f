// sr::ThinDisk's Doppler and redshift shading through the C++ host mirror
// (include/geo/sr.hpp): one small frame of the sky sphere with its thin disk,
// unshaded, shaded (set_shift) and unshaded again (clear_shift); FNV-1a of
// each.  tests/test_cpp_thin_disk_shift.py compares them with the CPU path's
// frames (geo_render_cpu_disk_shift).
//
//   sr_thin_disk_shift W H SPIN EXPONENT GAIN
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
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s W H SPIN EXPONENT GAIN\n", argv[0]);
        return 2;
    }
    try {
        sr::Renderer renderer((uint32_t)std::atoi(argv[1]), (uint32_t)std::atoi(argv[2]), 1.0, sr::kPi / 2);
        renderer.observer().set_position({2.4, 0.0, 0.7});
        sr::BasicSphereBuffer sky(0, 50.0, 1.0, pattern(512, 256), GEO_MODE_DIRECT, 2048);
        sky.update_ray_fan(renderer.get_radial_position());
        sr::ThinDisk disk;
        disk.texture = pattern(64, 16);
        disk.r_in = 1.6f;
        disk.r_out = 2.2f;
        const uint64_t plain = draw(renderer, sky, disk);
        disk.set_shift(std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]), (float)std::atof(argv[5]));
        const uint64_t shaded = draw(renderer, sky, disk);
        const uint64_t cleared = draw(renderer, sky, disk.clear_shift());
        std::printf("disk fnv1a %016llx\ndisk+shift fnv1a %016llx\ndisk cleared fnv1a %016llx\n",
                    (unsigned long long)plain, (unsigned long long)shaded, (unsigned long long)cleared);
        return 0;
    } catch (const sr::Error& e) {
        std::fprintf(stderr, "sr::Error: %s\n", e.what());
        return 3;
    }
}
