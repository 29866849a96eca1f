// sr::ThinDisk's blackbody emission through the C++ host mirror
// (include/geo/sr.hpp): one small frame of the sky sphere with its thin disk,
// unshaded, with the emission (set_emission) and unshaded again
// (clear_emission); FNV-1a of each.  tests/test_cpp_thin_disk_emission.py
// compares them with the CPU path's frames (geo_render_cpu_disk_emission).
//
//   sr_thin_disk_emission W H SPIN PROFILE T_REF T_LO T_HI EXPOSURE N
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

// a synthetic ramp of n entries: R falls, B rises, G a sawtooth
std::vector<uint8_t> ramp_of(uint32_t n) {
    std::vector<uint8_t> r((size_t)n * 4);
    for (uint32_t i = 0; i < n; ++i) {
        r[4 * i] = (uint8_t)(255u - 255u * i / (n - 1u));
        r[4 * i + 1] = (uint8_t)(i * 37u);
        r[4 * i + 2] = (uint8_t)(255u * i / (n - 1u));
        r[4 * i + 3] = 255;
    }
    return r;
}

uint64_t draw(sr::Renderer& renderer, sr::BasicSphereBuffer& sky, const sr::ThinDisk& disk) {
    sky.set_thin_disk(disk);
    renderer.render({&sky}, {});
    return fnv1a(renderer.read_frame());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s W H SPIN PROFILE T_REF T_LO T_HI EXPOSURE N\n", argv[0]);
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
        disk.set_emission(ramp_of((uint32_t)std::atoi(argv[9])), (float)std::atof(argv[5]), (float)std::atof(argv[6]),
                          (float)std::atof(argv[7]), (uint32_t)std::atoi(argv[4]), (float)std::atof(argv[8]),
                          std::atoi(argv[3]));
        const uint64_t emitting = draw(renderer, sky, disk);
        const uint64_t cleared = draw(renderer, sky, disk.clear_emission());
        std::printf("disk fnv1a %016llx\ndisk+emission fnv1a %016llx\ndisk cleared fnv1a %016llx\n",
                    (unsigned long long)plain, (unsigned long long)emitting, (unsigned long long)cleared);
        return 0;
    } catch (const sr::Error& e) {
        std::fprintf(stderr, "sr::Error: %s\n", e.what());
        return 3;
    }
}
