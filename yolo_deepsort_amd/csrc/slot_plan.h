// The slot plan of a detector pass whose frames are not one plain stack.  Plain C++: no device call, no device header.
//
// A slot is one network input: a th x tw region of the frames buffer stretched to the network size - a whole frame of any size, or
// one sliding window of a frame (ImageDetector(win_size, overlap), img_detect.py:97-151).  A plan lists the slots of a step in frame
// order, a windowed frame's in window order, and one NMS descriptor per frame.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace yds {

// One frame of a step whose frames differ in size (the "mixed" entries): h x w pixels at frames + off, rows w * 3 bytes apart.
struct FrameGeom { uint64_t off; int32_t h, w; };
// A slot's source region is th x tw pixels at frames + off (the window origin inside the frames buffer), rows `stride` bytes apart.
// window != 0: its boxes go to corner form, are scaled by (sx, sy) = (tw / img_w, th / img_h) and shifted by (x0, y0)
// (img_detect.py:132-138); else the network's rows are taken as they are.
struct SlotRec { uint64_t off; int32_t stride, th, tw, window, x0, y0; float sx, sy; };
// One frame of a ragged NMS launch: rows [row0, row0 + n_rows) of the prediction block; corner: they hold x1,y1,x2,y2; merge: the merge
// branch runs for it; (sx, sy): resize_boxes scale of its kept boxes (1 for a windowed frame, whose boxes are in frame pixels already).
struct NmsFrame { uint64_t row0; int32_t n_rows, corner, merge; float sx, sy; int32_t pad; };
// ImageDetector(win_size = (w, h), overlap); w <= 0: no setting
struct WindowSetting { int w = 0, h = 0; double overlap = 0; };

// resize_boxes (model_build.py:12-19): python-double ratio, one rounding to fp32
inline float box_scale(int frame_side, int net_side) { return (float)((double)frame_side / net_side); }
// window (x, y, th, tw) of a frame w pixels wide that starts at byte frame_off
inline SlotRec window_slot(uint64_t frame_off, int w, int x, int y, int th, int tw, int img_h, int img_w) {
    return SlotRec{frame_off + ((uint64_t)y * w + x) * 3, w * 3, th, tw, 1, x, y, box_scale(tw, img_w), box_scale(th, img_h)};
}
inline SlotRec plain_slot(uint64_t frame_off, int h, int w) { return SlotRec{frame_off, w * 3, h, w, 0, 0, 0, 1.f, 1.f}; }

struct SlotPlan {
    std::vector<SlotRec> slots;
    std::vector<NmsFrame> frames;
    int max_rows = 0;                  // largest n_rows of a frame
    bool windowed = false;             // some frame is cut into windows
    bool empty() const { return slots.empty(); }         // the plain uniform pass: no plan
    bool direct() const { return !empty() && !windowed; } // one plain slot per frame: slot b = frame b, the network's output is the prediction block
    bool operator==(const SlotPlan &o) const {
        if (slots.size() != o.slots.size() || frames.size() != o.frames.size()) return false;
        for (size_t n = 0; n < slots.size(); ++n) {                 // (the scales follow from th, tw)
            const SlotRec &a = slots[n], &b = o.slots[n];
            if (a.off != b.off || a.stride != b.stride || a.th != b.th || a.tw != b.tw || a.window != b.window || a.x0 != b.x0 || a.y0 != b.y0) return false;
        }
        for (size_t n = 0; n < frames.size(); ++n)
            if (frames[n].n_rows != o.frames[n].n_rows || frames[n].corner != o.frames[n].corner) return false;
        return true;
    }
};

// The plan of a step of n frames.  Layout: geom == nullptr - every frame h x w, frame b at byte b * h * w * 3; else frame b is geom[b]
// (h, w not used).  Window setting of frame b: win[b] when win holds n entries, win[0] for every frame when it holds one, none when
// it is empty.  A frame with a setting is cut by the reference's grid (img_detect.py:101-121: x-major, then y; each window extended by
// int(win * overlap) and clipped to the frame) unless w < win_w and h < win_h (img_detect.py:68: the plain branch).  A windowed frame's
// rows are in corner form in frame pixels (merge branch, scale 1), a plain frame's as the network gave them (centre form, the frame's
// own ratio).  Empty: a uniform layout without a windowed frame.
inline SlotPlan build_slot_plan(int n, int h, int w, const FrameGeom *geom, const std::vector<WindowSetting> &win, int img_h, int img_w,
                                int total_boxes) {
    SlotPlan pl;
    if (!geom && win.empty()) return pl;
    for (int b = 0; b < n; ++b) {
        const int fh = geom ? geom[b].h : h, fw = geom ? geom[b].w : w;
        const uint64_t off = geom ? geom[b].off : (uint64_t)b * fh * fw * 3;
        const WindowSetting sw = win.empty() ? WindowSetting() : win[win.size() == 1 ? 0 : b];
        NmsFrame f{(uint64_t)pl.slots.size() * total_boxes, 0, 0, 0, 1.f, 1.f, 0};
        if (sw.w > 0 && !(fw < sw.w && fh < sw.h)) {
            const int ox = (int)(sw.w * sw.overlap), oy = (int)(sw.h * sw.overlap);
            for (int x = 0; x < fw; x += sw.w)
                for (int y = 0; y < fh; y += sw.h) {
                    pl.slots.push_back(window_slot(off, fw, x, y, std::min(y + sw.h + oy, fh) - y, std::min(x + sw.w + ox, fw) - x, img_h, img_w));
                    f.n_rows += total_boxes;
                }
            f.corner = f.merge = 1;
            pl.windowed = true;
        } else {
            pl.slots.push_back(plain_slot(off, fh, fw));
            f.n_rows = total_boxes;
            f.sx = box_scale(fw, img_w);
            f.sy = box_scale(fh, img_h);
        }
        pl.max_rows = std::max(pl.max_rows, (int)f.n_rows);
        pl.frames.push_back(f);
    }
    if (!geom && !pl.windowed) return SlotPlan();
    return pl;
}

}  // namespace yds
