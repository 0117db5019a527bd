// Test-only driver of rtl-ws_amd/csrc/twiddle_tables.cpp (tests/test_tables_cpu.py): writes every
// non-empty table of tables_f32(N) and tables_f64(N) to DIR/<f32|f64>_<table>_<N>.bin.
//   dump_tables DIR N...
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "twiddle_tables.h"

template <typename V> static bool dump(const std::string& dir, const char* prec, const char* name, int n, const std::vector<V>& v)
{
    if (v.empty()) return true;
    const std::string path = dir + "/" + prec + "_" + name + "_" + std::to_string(n) + ".bin";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(V), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

static bool dump_all(const std::string& dir, const char* prec, int n, const rtlws::HostTables& h)
{
    return dump(dir, prec, "tw1", n, h.tw1) && dump(dir, prec, "tw1_128", n, h.tw1_128) &&
           dump(dir, prec, "tw2", n, h.tw2) && dump(dir, prec, "hann_cs", n, h.hann_cs) &&
           dump(dir, prec, "hann", n, h.hann) && dump(dir, prec, "tw64", n, h.tw64) &&
           dump(dir, prec, "hann64", n, h.hann64) && dump(dir, prec, "tw1_64", n, h.tw1_64) &&
           dump(dir, prec, "tw1u_64", n, h.tw1u_64) && dump(dir, prec, "tw2_64", n, h.tw2_64) &&
           dump(dir, prec, "hann_cs64", n, h.hann_cs64) && dump(dir, prec, "twxa_64", n, h.twxa_64) &&
           dump(dir, prec, "twxb_64", n, h.twxb_64);
}

int main(int argc, char** argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: dump_tables DIR N...\n");
        return 2;
    }
    for (int i = 2; i < argc; ++i) {
        const int n = atoi(argv[i]);
        if (!dump_all(argv[1], "f32", n, rtlws::tables_f32(n)) || !dump_all(argv[1], "f64", n, rtlws::tables_f64(n))) {
            fprintf(stderr, "dump_tables: cannot write to %s\n", argv[1]);
            return 1;
        }
    }
    return 0;
}
