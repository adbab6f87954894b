// The coloured PLY writer of host/lgr_io.hpp, driven by tests/test_formats_colored.py, which wrote the same cloud with
// lgr_amd/formats.py write_ply_colored and compares the files byte for byte.  No GPU, no library call.
//   colored_ply_write <dir>     <dir>/cloud.bin: int32 n, n x 12 float32 rows, n int32 colours  ->  <dir>/cpp_bin.ply, <dir>/cpp_ascii.ply
#include <cstdio>
#include <fstream>

#include "../../lidar-global-registration_amd/host/lgr_io.hpp"

using namespace lgr;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = std::string(argv[1]) + "/";
    std::ifstream f(d + "cloud.bin", std::ios::binary);
    std::int32_t n = 0;
    f.read(reinterpret_cast<char*>(&n), 4);
    std::vector<float> rows(static_cast<std::size_t>(n) * 12);
    std::vector<std::int32_t> colors(static_cast<std::size_t>(n));
    f.read(reinterpret_cast<char*>(rows.data()), static_cast<std::streamsize>(rows.size() * 4));
    f.read(reinterpret_cast<char*>(colors.data()), static_cast<std::streamsize>(colors.size() * 4));
    if (!f.good()) return 1;
    PointColoredNCloud cloud;
    cloud.points.resize(static_cast<std::size_t>(n));
    for (std::int32_t i = 0; i < n; ++i) {
        PointN p;
        std::memcpy(static_cast<void*>(&p), &rows[static_cast<std::size_t>(i) * 12], 48);
        copyPoint(p, cloud.points[static_cast<std::size_t>(i)]);
        setPointColor(cloud.points[static_cast<std::size_t>(i)], colors[static_cast<std::size_t>(i)]);
    }
    if (savePLYFileBinary(d + "cpp_bin.ply", cloud) < 0 || savePLYFileASCII(d + "cpp_ascii.ply", cloud) < 0) return 1;
    // mixPointColor applied 0 to 3 times to red, and getColor at the ends of a range
    PointColoredN q;
    setPointColor(q, COLOR_RED);
    for (int k = 0; k < 4; ++k) { std::printf("mix%d %02x%02x%02x\n", k, q.r, q.g, q.b); mixPointColor(q, COLOR_WHITE); }
    std::printf("color %06x %06x %06x\n", getColor(0.f, 0.f, 1.f), getColor(1.f, 0.f, 1.f), getColor(0.5f, 0.f, 1.f));
    std::vector<float> v{0.5f, 1.25f, 1e-7f};
    saveVector(v, d + "cpp_vector.csv");
    return 0;
}
