// The histogram and extracted-id writers of the C++ header (lgr_io.hpp: saveFeatures, featuresStem, saveExtractedPointIds), driven by
// tests/test_prepared_formats.py, which wrote the same tables with lgr_amd/formats.py and compares the files byte for byte.  No GPU, no
// library call.
//   prepared_formats <dir>
//     <dir>/rows.bin (int32 n, int32 row_len, n x row_len floats)     -> cpp_<featuresStem>.csv, once with the row numbers, once with indices
//     <dir>/ids.bin  (int32 n, n x {int32 id_src, id_tgt}, then two clouds of n_src / n_tgt x 3 floats, each after its int32 size)
//                                                                      -> cpp_ids.csv
#include <cstdio>
#include <fstream>

#include "../../lidar-global-registration_amd/host/lgr_io.hpp"

using namespace lgr;

static std::int32_t read_i32(std::ifstream& f) { std::int32_t v = 0; f.read(reinterpret_cast<char*>(&v), 4); return v; }

static PointNCloud read_cloud(std::ifstream& f) {
    PointNCloud c;
    const std::int32_t n = read_i32(f);
    c.points.resize((std::size_t) n);
    for (PointN& p : c.points) {
        float xyz[3];
        f.read(reinterpret_cast<char*>(xyz), 12);
        p.x = xyz[0]; p.y = xyz[1]; p.z = xyz[2];
    }
    return c;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = std::string(argv[1]) + "/";
    std::ifstream fr(d + "rows.bin", std::ios::binary);
    const std::int32_t n = read_i32(fr), len = read_i32(fr);
    std::vector<float> rows((std::size_t) n * (std::size_t) len);
    fr.read(reinterpret_cast<char*>(rows.data()), (std::streamsize) (rows.size() * 4));
    if (!fr) return 1;
    saveFeatures(rows.data(), (std::size_t) n, (std::size_t) len, nullptr, d + "cpp_" + featuresStem(true) + ".csv");
    std::vector<int> indices;
    for (int i = 0; i < n; ++i) indices.push_back(1000 - 7 * i);
    saveFeatures(rows.data(), (std::size_t) n, (std::size_t) len, &indices, d + "cpp_" + featuresStem(false, -3) + ".csv");
    std::printf("%s %s %s\n", featuresStem(true).c_str(), featuresStem(false).c_str(), featuresStem(true, 2).c_str());

    std::ifstream fi(d + "ids.bin", std::ios::binary);
    const std::int32_t m = read_i32(fi);
    std::vector<int> src_ids, tgt_ids;
    for (int i = 0; i < m; ++i) { src_ids.push_back(read_i32(fi)); tgt_ids.push_back(read_i32(fi)); }
    const PointNCloud src = read_cloud(fi), tgt = read_cloud(fi);
    if (!fi) return 1;
    saveExtractedPointIds(src_ids, tgt_ids, src, tgt, d + "cpp_ids.csv");
    return 0;
}
