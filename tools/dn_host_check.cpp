// Stand-alone check of the host-only parts of the file-level flow (babe_amd/csrc/dn_host.h), for a host compiler with sanitizers:
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o dn_host_check tools/dn_host_check.cpp
//     dn_host_check table ORIG NEW          width orig new_, then per phase: first last, then the taps as hexadecimal floats
//     dn_host_check length L ORIG NEW       the resampled length
//     dn_host_check walk N SEGMENT OVERLAP  the number of segments (or -1), then their starts
//     dn_host_check rates L FS FS_DN FS_MODEL   the conversion mask and the three lengths
//     dn_host_check files FILE...           per file "FILE: ok (...)" or "FILE: refused: MESSAGE", as babe_denoiser_load judges it
// Tables and walks are written into heap buffers of exactly their size, files are read into one, so that a step past an end is a
// sanitizer report.  Exit status 0 whatever the verdicts are; 2 for bad usage or a file that cannot be read.
// tests/test_dn_library_cpu.py compares every answer with the library's.
#include "../babe_amd/csrc/dn_host.h"

#include <cstdlib>

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    auto num = [&](int i) { return atol(argv[i]); };
    if (cmd == "table" && argc == 4) {
        babe_dn::SincDims d;
        if (!babe_dn::sinc_dims(num(2), num(3), d)) return printf("refused\n"), 0;
        const size_t taps = (size_t)2 * d.width + d.orig;
        float* kernel = static_cast<float*>(malloc(taps * d.new_ * sizeof(float)));
        int* krange = static_cast<int*>(malloc((size_t)2 * d.new_ * sizeof(int)));
        if (!kernel || !krange) return 2;
        babe_dn::sinc_table(d, kernel, krange);
        printf("%d %d %d\n", d.width, d.orig, d.new_);
        for (int j = 0; j < d.new_; ++j) {
            printf("%d %d", krange[2 * j], krange[2 * j + 1]);
            for (size_t k = 0; k < taps; ++k) printf(" %a", (double)kernel[j * taps + k]);
            printf("\n");
        }
        free(kernel), free(krange);
    } else if (cmd == "length" && argc == 5) {
        printf("%ld\n", babe_dn::resampled_length(num(2), num(3), num(4)));
    } else if (cmd == "walk" && argc == 5) {
        const long count = babe_dn::denoise_plan(num(2), num(3), num(4), nullptr, 0);
        printf("%ld", count);
        if (count > 0) {
            long* starts = static_cast<long*>(malloc((size_t)count * sizeof(long)));
            if (!starts) return 2;
            babe_dn::denoise_plan(num(2), num(3), num(4), starts, count);
            for (long j = 0; j < count; ++j) printf(" %ld", starts[j]);
            free(starts);
        }
        printf("\n");
    } else if (cmd == "rates" && argc == 6) {
        long* lengths = static_cast<long*>(malloc(3 * sizeof(long)));
        if (!lengths) return 2;
        lengths[0] = lengths[1] = lengths[2] = 0;
        const int mask = babe_dn::file_plan(num(2), num(3), num(4), num(5), lengths);
        printf("%d %ld %ld %ld\n", mask, lengths[0], lengths[1], lengths[2]);
        free(lengths);
    } else if (cmd == "files") {
        for (int i = 2; i < argc; ++i) {
            FILE* fh = fopen(argv[i], "rb");
            if (!fh) return fprintf(stderr, "%s: cannot open\n", argv[i]), 2;
            fseek(fh, 0, SEEK_END);
            const long size = ftell(fh);
            fseek(fh, 0, SEEK_SET);
            unsigned char* buf = static_cast<unsigned char*>(malloc(size > 0 ? (size_t)size : 1));
            if (size < 0 || !buf || fread(buf, 1, (size_t)size, fh) != (size_t)size) return fprintf(stderr, "%s: cannot read\n", argv[i]), 2;
            fclose(fh);
            {
                babe_model::File f;
                babe_dn::DnCfg cfg;
                std::string err;
                if (babe_model::parse(size > 0 ? buf : nullptr, (size_t)size, f, err) && babe_dn::dn_validate(f, cfg, err)) {
                    double sum = 0;                   // touch every byte the table points at
                    for (const babe_model::Tensor& t : f.tensors)
                        for (size_t k = 0; k < t.numel; ++k) sum += t.data[k];
                    printf("%s: ok (%zu tensors, %zu settings, segment %ld, checksum %.6g)\n", argv[i], f.tensors.size(), f.settings.size(), cfg.segment, sum);
                } else {
                    printf("%s: refused: %s\n", argv[i], err.c_str());
                }
            }
            free(buf);
        }
    } else {
        return 2;
    }
    return 0;
}
