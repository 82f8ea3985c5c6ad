// lds_layout.hpp — geometry of the small kernels' LDS emission tables (hmmbw_device.hpp): the row layout's
// table distance and sizes, and the address functions of the class-split layout (LAY = 1).
// Plain constexpr C++ with no HIP dependency, so that a host compiler can build a probe of them
// (tests/native/lds_layout_probe.cpp).
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define HMMBW_HD __host__ __device__
#else
#define HMMBW_HD
#endif

namespace hmmbw {

// The row layout (LAY = 0): two [K][G] tables of 16-B entries, the H-table kHistOff bytes after the P-table.
// The kernels use them when the P-table fits below kHistOff (the row offsets then fit the uint16 symbol packs).
constexpr int kHistOff = 32768;
HMMBW_HD constexpr bool lds_tables_fit(int K, int GP) { return (size_t)K * GP * 16 <= (size_t)kHistOff; }
HMMBW_HD constexpr size_t lds_table_bytes(int K, int GP) { return (size_t)kHistOff + (size_t)K * GP * 16; }

// The class-split layout (LAY = 1) of the joined map's G = 8 kernels (k_estep_join<.., 1>), which own a whole
// CU's LDS.  In the row layout (hmmbw_device.hpp) a ds_read_b128 lane group ({0-3, 12-15, 20-27}, ... MI355X: four 16-B windows
// of four states, of sequence slots 0, 1, 2, 3) puts slots 0 and 3 (states 0-3) and slots 1 and 2 (states 4-7)
// on the same 16 banks whenever their symbols have equal parity: 1.74 LDS cycles per group on uniform symbols
// (tools/lds_banks.py).  Here slot u reads the tables of its class (u >> 1) & 1, and each class owns K rows of
//   [ P row: GP x {x, y} | H row: GP x {h, b} ]            (2 GP 16 bytes, 256 for G = 8)
// with class 1's region 65,536 + GP 16 bytes after class 0's, so class 0's P rows lie on banks 0-31 of the
// read's 64 and class 1's on banks 32-63: the four windows of a lane group fall on four different bank
// quarters whatever the symbols (1.00 cycles per group).  The packs hold o 2 GP 16 (<= 65,280 at K = 256:
// uint16 still), the lane's base adds the class offset once per wave, and H - P is the constant GP 16, the
// immediate offset of the histogram add and the H.b read: the per-step instructions are those of layout 0.
// Both classes hold the same P and b; each accumulates its own slots' histogram h, summed at the flush.
HMMBW_HD constexpr int lay2_row_bytes(int GP) { return 2 * GP * 16; }
HMMBW_HD constexpr int lay2_hist_off(int GP) { return GP * 16; }  // H entry - P entry
HMMBW_HD constexpr int lay2_class_off(int GP) { return 65536 + GP * 16; }
// class of sequence slot u: slots 0|3 and 1|2 of a read group apart; the two slots 2i, 2i + 1 of a ds_add_f64 lane
// group together, so their adds meet as in layout 0 (u & 1 would cost skewed symbols a second add cycle in the model)
HMMBW_HD constexpr int lay2_class(int u) { return (u >> 1) & 1; }
HMMBW_HD constexpr bool lay2_tables_fit(int K, int GP) { return (size_t)K * lay2_row_bytes(GP) <= 65536; }
HMMBW_HD constexpr size_t lay2_table_bytes(int K, int GP) {
    return (size_t)lay2_class_off(GP) + (size_t)K * lay2_row_bytes(GP);
}
// byte offset of the P entry of (class, symbol o, state column j); the pack entry of symbol o is lay2_p_off(GP, 0, o, 0)
HMMBW_HD constexpr size_t lay2_p_off(int GP, int cls, int o, int j) {
    return (size_t)cls * lay2_class_off(GP) + (size_t)o * lay2_row_bytes(GP) + (size_t)j * 16;
}

}  // namespace hmmbw
