// cdist_dev.h -- what the matrix-core kernels over pairs of rows share on the device (cdist.hip, nearest.hip): the geometry of a K-tile per
// storage type, the load of one staged item and the squares it adds to a row's partial norm.  The ORDER of those additions is part of the
// C-ABI (include/si_cdist.h, restated by tests/cdist_reference.py mm_sqnorm); it is written here, once.  Included after si_hip_internal.h by a
// file that has switched contraction off.
#ifndef SI_CDIST_DEV_H_
#define SI_CDIST_DEV_H_

// ---- the mm kernel's geometry per storage type: elements of an item (the 16-byte K vector), of a K-tile (8 items) and the LDS row pitch
template <typename T> struct CdMm;
template <> struct CdMm<float> {
    typedef f32x4 item_t;
    static constexpr int VW = 4, BK = SI_G64_BK, LDL = SI_G64_LDL, LDS_ELEMS = SI_G64_LDS_FLOATS;
};
template <> struct CdMm<_Float16> {
    typedef f16x8 item_t;
    // 64 + 8 halves: rows 144 bytes apart, so the 16 rows of a fragment read start 36 words apart (4 banks) and a 16-byte read per lane
    // covers the banks evenly
    static constexpr int VW = 8, BK = 64, LDL = 64 + 8, LDS_ELEMS = (SI_G64_BM + SI_G64_BN) * LDL;
};

// one item of row `row` (of `rows`) at element k: zeros beyond the rows, and element by element beyond m in the single-element form
template <typename T, bool VEC>
__device__ __forceinline__ typename CdMm<T>::item_t cd_load_item(const T* base, int row, int rows, int ld, int k, int m) {
    typedef typename CdMm<T>::item_t item_t;
    item_t v;
#pragma unroll
    for (int j = 0; j < CdMm<T>::VW; ++j) v[j] = (T)0;
    if (row < rows && k < m) {
        const T* const p = base + (size_t)row * ld + k;
        if (VEC) {
            v = *reinterpret_cast<const item_t*>(p);
        } else {
#pragma unroll
            for (int j = 0; j < CdMm<T>::VW; ++j)
                if (k + j < m) v[j] = p[j];
        }
    }
    return v;
}

// q += the squares of an item's elements, in k order, each square rounded on its own
template <typename Item, int VW>
__device__ __forceinline__ float cd_add_squares(float q, const Item& v) {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
        const float e = (float)v[j];
        q = q + e * e;
    }
    return q;
}

#endif  // SI_CDIST_DEV_H_
