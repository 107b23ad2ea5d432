// Host run of label_crops_kernel (csrc/crops.hip) for tests/test_crops_kernel_host_cpu.py: the kernel's own text, cut out of crops.hip by the
// test into KERNEL_TEXT, compiled as plain C++ with the shims below and run thread by thread, every buffer an exact-size heap block, so that
// the address and undefined-behaviour sanitizers of the host compiler see any tap or store outside its buffer and any overflow of the
// position arithmetic.  No GPU, no HIP.
//   crops_kernel_host IN OUT
// IN:  int32 ncases, then per case int32 {nimg, H, W, C, elem_bytes, m, OH, OW, flags, fill, has_image, has_masks, grid}, the labels, the
//      image (if any), the jobs.  OUT: per case the patches (if any) and the masks (if any), as the kernel left them over a 0xA5 fill.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct Dim { unsigned x; };
static Dim threadIdx, blockIdx, gridDim;
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#include KERNEL_TEXT

template <typename T>
static void run(const int* labels, int nimg, int H, int W, const T* image, int C, const int* jobs, long m, int OH, int OW, int flags, unsigned fill,
                T* patches, unsigned char* masks, unsigned grid) {
    const int nchunk = (OH * OW + KG_CROPS_CHUNK - 1) / KG_CROPS_CHUNK;    // as the entry launches it
    const long items = m * nchunk;
    const bool nearest = (flags & KG_CROPS_NEAREST) != 0 || !patches;
    const int masked = (flags & KG_CROPS_MASKED) != 0;
    gridDim.x = grid;
    for (unsigned b = 0; b < grid; ++b)
        for (unsigned t = 0; t < 256; ++t) {
            blockIdx.x = b; threadIdx.x = t;
            if (nearest) label_crops_kernel<T, true>(labels, nimg, H, W, image, C, jobs, items, nchunk, OH, OW, masked, fill, patches, masks);
            else label_crops_kernel<T, false>(labels, nimg, H, W, image, C, jobs, items, nchunk, OH, OW, masked, fill, patches, masks);
        }
}

static void* take(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short input\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 2;
    for (int c = 0; c < ncases; ++c) {
        int h[13];
        if (fread(h, 4, 13, f) != 13) return 2;
        const int nimg = h[0], H = h[1], W = h[2], C = h[3], eb = h[4], m = h[5], OH = h[6], OW = h[7], flags = h[8], fill = h[9], has_img = h[10],
                  has_masks = h[11], grid = h[12];
        const size_t px = (size_t)nimg * H * W;
        int* labels = (int*)take(f, px * 4);
        void* image = has_img ? take(f, px * C * eb) : nullptr;
        int* jobs = (int*)take(f, (size_t)m * 40);
        const size_t pb = has_img ? (size_t)m * C * OH * OW * eb : 0, mb = has_masks ? (size_t)m * OH * OW : 0;
        void* patches = pb ? malloc(pb) : nullptr;
        unsigned char* masks = mb ? (unsigned char*)malloc(mb) : nullptr;
        if (patches) memset(patches, 0xA5, pb);
        if (masks) memset(masks, 0xA5, mb);
        if (eb == 2)
            run<unsigned short>(labels, nimg, H, W, (const unsigned short*)image, has_img ? C : 1, jobs, m, OH, OW, flags, (unsigned)fill,
                                (unsigned short*)patches, masks, (unsigned)grid);
        else
            run<unsigned char>(labels, nimg, H, W, (const unsigned char*)image, has_img ? C : 1, jobs, m, OH, OW, flags, (unsigned)fill,
                               (unsigned char*)patches, masks, (unsigned)grid);
        if (pb) fwrite(patches, 1, pb, o);
        if (mb) fwrite(masks, 1, mb, o);
        free(labels); free(image); free(jobs); free(patches); free(masks);
    }
    fclose(f);
    fclose(o);
    return 0;
}
