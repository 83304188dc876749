/* trsim_spec.h — the frozen numerical specification of the batched env.
 *
 * The reference (Triton-AI/Triton-Racer-Sim) holds NO vehicle dynamics and NO
 * camera renderer: TritonRacerSim/components/gyminterface.py:47-104 is a TCP
 * client of an external closed Unity binary.  Everything
 * in this header is therefore a build-defined free parameter (SURVEY.md
 * Appendix B).  It is the single source of truth for CONSTANTS ONLY; the HIP
 * library (triton-racer-sim_amd/csrc) and the CPU oracle (oracle/) implement
 * the arithmetic below independently, from this text, and must agree
 * bit-for-bit (integer results) / within 1e-5 (pose, speed).
 *
 * Arithmetic rules (both implementations):
 *   R1  all env state is IEEE-754 binary32; add/sub/mul/div/sqrt correctly
 *       rounded; NO floating-point contraction (-ffp-contract=off); an FMA is
 *       used only where the spec writes fma(a,b,c).
 *   R2  sin/cos come from trs_sincos below (never libm / device intrinsics).
 *   R3  the nearest-point search (reference LocationTracker,
 *       TritonRacerSim/components/track_data_process.py:89-104) runs in
 *       binary64 on the binary64 track points: d_i = (|x-xi| + |y-yi|) + |z-zi|,
 *       best initialised to 100.0, strict '<', lowest index wins.
 *       An implementation may first scan only the points of the 3x3 block of TRS_NEAR_GRID_CELL-sized (x, z) cells around
 *       the query: every point outside the block is at least one cell size away in x or z, so a block result with
 *       d < TRS_NEAR_GRID_CELL is the global result (no outside point can beat or tie it); otherwise it must scan all points.
 *
 * ---- trs_sincos(a), |a| <= pi + 1e-3 -------------------------------------
 *   q  = rint(a * TRS_TWO_OVER_PI)              (round-half-even)
 *   r  = fma(q, -TRS_PIO2_HI, a);  r = fma(q, -TRS_PIO2_LO, r)
 *   z  = r*r
 *   ps = fma(fma(TRS_S0, z, TRS_S1), z, TRS_S2)        sin: s = fma(r*z, ps, r)
 *   pc = fma(fma(TRS_C0, z, TRS_C1), z, TRS_C2)        cos: c = fma(z*z, pc, fma(z, -0.5f, 1.0f))
 *   n  = ((int)q) & 3:  0:(s,c) 1:(c,-s) 2:(-s,-c) 3:(-c,s)
 *
 * ---- one env step (controls steer, thr, brk; state x,y,z,yaw,v) ----------
 *   steer = clamp(steer,-1,1); thr = clamp(thr,-1,1); brk = clamp(brk,0,1)
 *   (sd,cd) = trs_sincos(steer * max_steer);  tan_d = sd / cd
 *   a   = thr*accel_max - drag_lin*v
 *   v1  = v + a*dt
 *   dv  = (roll_res + brk*brake_max) * dt
 *   v2  = v1>0 ? max(v1-dv,0) : (v1<0 ? min(v1+dv,0) : 0);  v2 = clamp(v2,-v_rev_max,v_max)
 *   yaw1 = yaw + ((v2*tan_d)*inv_wheelbase)*dt;  if yaw1> PI: yaw1-=TWO_PI; if yaw1<-PI: yaw1+=TWO_PI
 *   (s,c) = trs_sincos(yaw1)           heading: forward = (s, c) in (x, z); Unity y-up, left-handed
 *   x1 = x + (v2*s)*dt;   z1 = z + (v2*c)*dt
 *   idx = L1 nearest raw track point of ((double)x1,(double)y,(double)z1)        [R3]
 *   y1  = (float)Py[idx]
 *   cte = (x1-(float)Px[idx])*tz[idx] - (z1-(float)Pz[idx])*tx[idx]   (+ = right of the centre line)
 *   lost = (best_d >= 100.0);  done = |cte| > offtrack_cte || lost
 *   d = idx - prev_idx wrapped to [-n/2, n/2);  reward = (float)d - (done ? offtrack_penalty : 0)
 *   ep_return += reward; ep_len += 1
 *   reset (usr/reset truthy, or auto_reset && previous done): state := start pose of the env,
 *   no integration this step, reward 0, last_return := ep_return, ep_return := 0, ep_len := 0.
 *
 * ---- class map (the track surface the camera sees; built on the host in binary64) ----
 *   polyline Q: the raw track points in (x, z), consecutive equal points dropped, a closing duplicate of the first dropped;
 *     it is CLOSED: m points, m segments Q[k] -> Q[(k+1) mod m]; s_k = sum of the lengths of segments 0..k-1.
 *   grid: cell = TRS_MAP_CELL_MIN * 2^j with the smallest j >= 0 for which the packed map fits TRS_MAP_LDS_BUDGET:
 *     x0 = floor((min x of Q - map_margin) / cell) * cell,  GW = ceil((max x of Q + map_margin - x0) / cell);  z0, GH likewise;
 *     MW = ceil(GW / 16) 32-bit words per row (16 cells of 2 bits, cell ix in bits 2*(ix mod 16)..+1 of word ix / 16);
 *     it fits when MW * 4 * GH <= TRS_MAP_LDS_BUDGET.
 *   cell (ix, iz), centre c = (x0 + (ix + 0.5) * cell, z0 + (iz + 0.5) * cell):
 *     per segment k: t = clamp(((c - Q[k]) . (Q[k+1] - Q[k])) / |Q[k+1] - Q[k]|^2, 0, 1), foot = Q[k] + t (Q[k+1] - Q[k])
 *     d   = min over k of |c - foot_k|  (Euclidean), taken at the LOWEST k that attains it
 *     arc = s_k + t_k * |Q[k+1] - Q[k]| at that k  (arc length along the centre line)
 *     class = CENTRE  if d <= centre_half and fmod(arc, dash_period) < dash_on      (dashed centre line)
 *             EDGE    else if |d - road_half| <= edge_half                           (solid edge lines, centred on the road edge)
 *             ROAD    else if d < road_half
 *             GRASS   otherwise
 *     the outermost ring of cells (ix = 0, GW-1 or iz = 0, GH-1) is GRASS whatever the rule says: lookups that fall outside
 *     the map are clamped onto it.  (A builder may skip segments farther from a cell than road_half + edge_half + cell:
 *     they cannot change the class.)
 *   An independent numpy restatement of this paragraph checks both builders: tests/test_independent_spec.py.
 *
 * ---- camera (pinhole over the ground plane y = 0; no roll) ----------------
 *   per image row v (tables built on the host in binary64, stored binary32):
 *     f = (H/2)/tan(fov_v/2);  yn = (H/2-(v+0.5))/f
 *     dy = yn*cos(pitch)-sin(pitch);  dz = yn*sin(pitch)+cos(pitch)
 *     dy >= -1e-6            -> SKY row
 *     t = cam_h/(-dy); t*dz > z_far -> FAR row (fog colour)
 *     else GROUND row: row_lz[v] = t*dz/cell, row_k[v] = (t/f)/cell
 *   per env: camx = ((x1 + cam_fwd*s) - map_x0)*inv_cell, camz likewise with c, z1, map_z0
 *   per pixel (u,v): uf = (float)u + 0.5f - W/2
 *     ax = fma(row_lz[v], s, camx); az = fma(row_lz[v], c, camz)
 *     dx = row_k[v]*c;              dzz = -(row_k[v]*s)
 *     gx = fma(uf, dx, ax); gz = fma(uf, dzz, az)
 *     ix = clamp((int)floor(gx), 0, GW-1); iz = clamp((int)floor(gz), 0, GH-1)
 *     cls = 2-bit class of cell (ix, iz)  (the map border is class 0)
 *     rgb = palette[v][cls]
 *   SKY/FAR rows have row_lz = row_k = 0 and a palette whose 4 entries are equal.
 *   depth channel (optional, binary32 [H][W]): z-depth of the ground plane, constant along an image row:
 *     GROUND row: (float)(t*dz) world units;  SKY and FAR rows: (float)z_far.
 *
 * ---- tracks with elevation (round 5) -----------------------------------------
 *   The raw points carry a height y (reference car_templates/track_data/mountain_track.json: y in 3.19 .. 7.35).  A track is HILLY when
 *   max y - min y > TRS_HILL_MIN_RANGE; flat tracks (generated_track: 0.011) keep everything above, bit for bit.  On a hilly track the car
 *   stands on the road's local slope and looks at a road that tilts against it ahead: the camera is fixed to the car, so what changes in
 *   its image is the angle between its axis and the ground plane AHEAD.  The ground the camera sees is modelled as ONE plane per env and
 *   frame — through the camera's foot point, tilted against the car's own plane by the change of slope between the car's track point
 *   and a point TRS_HILL_AHEAD samples further on — i.e. the flat-ground camera above with a PER-ENV pitch (height cam_h and forward
 *   offset cam_fwd unchanged: the rotation is taken about the camera, a documented approximation).  Row tables and the fogged palette
 *   then depend on the env and the frame; they are evaluated in binary32 with the operation order below (host tables in binary64 as
 *   before):
 *   host, binary64, per raw point i (indices wrap, the track is closed):
 *     h_i     = horizontal length of the step from point i to point i+1:  sqrt((Px[i+1]-Px[i])^2 + (Pz[i+1]-Pz[i])^2)   (0 for duplicates)
 *     d_i     = h_{i-L} + h_{i-L+1} + ... + h_{i+L-1}    (the path from point i-L to point i+L, summed in this order), L = TRS_HILL_SPAN
 *     g_i     = d_i > 1e-9 ? (Py[i+L] - Py[i-L]) / d_i : 0                      (smoothed grade)
 *     theta_i = atan(g_i)
 *     dpitch[i] = (float)clamp(theta_{i+A} - theta_i, -TRS_HILL_MAX_DPITCH, TRS_HILL_MAX_DPITCH),  A = TRS_HILL_AHEAD
 *     sky[v]  = the SKY colour of image row v as above, for EVERY row v (g = min((v+0.5)/(H/2), 1))
 *     far     = the FAR colour as above;  inv_f = (float)(1/f); hh = (float)(H/2); pitch_f = (float)pitch; cam_h_f, z_far_f = (float) of theirs;
 *     inv_zfar_f = (float)(1/z_far); inv_cell_f = (float)(1/cell) (exact); fog_f = (float)TRS_FOG_MAX; base / fog colours as binary32
 *   per env and frame, binary32 (R1: every operation rounded, no contraction), idx = the step's nearest raw track point:
 *     P = pitch_f + dpitch[idx];   (sp, cp) = trs_sincos(P)
 *     per image row v:  yn = (hh - ((float)v + 0.5f)) * inv_f;   dy = yn*cp - sp;   dz = yn*sp + cp
 *       dy >= -1e-6f                  -> SKY row:  row_lz = row_k = 0, depth z_far_f, the four class colours = sky[v]
 *       t = cam_h_f / (-dy);  zd = t*dz;  zd > z_far_f -> FAR row: row_lz = row_k = 0, depth z_far_f, colours = far
 *       else GROUND row: row_lz = zd * inv_cell_f;  row_k = (t * inv_f) * inv_cell_f;  depth = zd
 *            fw = fog_f * (zd * inv_zfar_f);  colour[c][ch] = (int)((base[c][ch] * (1.0f - fw) + fog[ch] * fw) + 0.5f)
 *     pixels exactly as above with these row tables.  The depth frame is constant along a row of one frame, and now differs from env to env
 *     and from frame to frame with the slope ahead.
 *
 * ---- lens camera (trs_set_camera; flat tracks only; parity with the simulator UNPINNED) ----------------------------------------------
 *   The reference's gym_config carries the donkey simulator's fish_eye_x, fish_eye_y and offset_x (gyminterface.py:16-45); the simulator is a
 *   closed binary and the reference's cam_config send is commented out (:136-152), so this model, like everything above, is defined by this build.
 *   kx = fish_eye_x, ky = fish_eye_y in [0, 2] (0 = pinhole); ox = offset_x in world units, + = right of the heading, |ox| <= 2.
 *   f, pitch, cam_h, z_far and the map cell as in the flat camera paragraph.  kx = ky = ox = 0 selects the flat camera above (not this path).
 *   per pixel (u, v), host, binary64:
 *     xn = ((u + 0.5) - W/2) / f;  yn = (H/2 - (v + 0.5)) / f
 *     rho2 = (((u + 0.5) - W/2)^2 + (H/2 - (v + 0.5))^2) / (H/2)^2
 *     xr = xn * (1 + kx*rho2);  yr = yn * (1 + ky*rho2)                    (k > 0: edge rays bend outward = barrel / fish-eye)
 *     dy = yr*cos(pitch) - sin(pitch);  dz = yr*sin(pitch) + cos(pitch)
 *     dy >= -1e-6 -> SKY: g = clamp((H/2 - yr*f) / (H/2), 0, 1); row S(min((int)(g*256), 255)); F = L = 0, depth = (float)z_far
 *     t = cam_h/(-dy); zd = t*dz;  zd > z_far -> FAR: row FAR; F = L = 0, depth = (float)z_far
 *     else GROUND: F = (float)(zd/cell), L = (float)((t*xr)/cell), depth = (float)zd, row G(clamp((int)(zd/z_far*256), 0, 255))
 *   lens palette, 513 rows of 4 class colours (host, binary64, the flat palette's rounding floor(x + 0.5)):
 *     G(q), q < 256: fw = TRS_FOG_MAX * ((q + 0.5)/256), colour[c] = base[c]*(1 - fw) + fog*fw;  S(q): the flat sky blend at g = (q + 0.5)/256,
 *     four equal colours;  FAR: the flat FAR colour.  A static frame filter applies to every entry, as to the flat palette.
 *   per env and frame, binary32 (R1): (camx, camz, s, c) exactly as the flat camera (cam_fwd included);  oc = (float)(ox/cell) (host)
 *     cx = fma(oc, c, camx);  cz = fma(oc, -s, camz)
 *   per pixel: gx = fma(L, c, fma(F, s, cx));  gz = fma(L, -s, fma(F, c, cz));  ix = clamp((int)floor(gx), 0, GW-1), iz likewise
 *     rgb = lens_palette[row][class(ix, iz)]  (SKY and FAR rows have four equal colours: their F = L = 0 lookup does not matter)
 *   depth frame: depth per pixel.  The offset stays out of the table: pixels u and W-1-u have bit-identical F, depth and row and exactly negated L
 *   (every binary64 operation sees identical or exactly negated operands), so a device may keep half of the table.
 *   An independent numpy restatement checks the host tables (tests/test_lens_tables_cpu.py); a C restatement of the per-pixel pass checks the
 *   frames (tests/test_lens_gpu.py).
 *
 * ---- scene lighting (trs_set_lighting; the pinhole camera on flat tracks and on tracks with elevation; not the lens camera) --------------------
 *   Per env e, binary32 gain[e][ch] and bias[e][ch] for ch = R, G, B (frame channel order), laid out as float[n_envs][8] {gR gG gB 0 bR bG bB 0}.
 *   Applied to the raw rendered colour of every pixel — after the fog blend and its rounding, before any frame filter — per channel x, binary32 (R1):
 *     t = (float)x * gain;  t = t + bias;  t = t + 0.5f
 *     out = !(t > 0.f) ? 0 : (t >= 255.f ? 255 : (int)t)                    (NaN -> 0)
 *   gain = 1, bias = 0 is the identity, bit for bit.  A function of the colour alone: a lit frame equals L_e(raw frame) pixel for pixel, and with
 *   a frame filter the frame equals filter(L_e(raw frame)) — with dynamic brightness, the frame's mean is the LIT frame's.  Depth, state, indices
 *   and returns are untouched.  Not defined here (refused): the lens camera.  tests/test_lighting_cpu.py restates the rule in numpy against the product's
 *   function (csrc/trsim_tables.hpp, light_channel); tests/test_lighting_gpu.py checks frames against the oracle's raw frames with the rule applied.
 *
 * ---- observation latency (trs_set_latency; sim_latency of the reference's gym_config, per env; HIP library only) --------------------------------
 *   The reference accepts a telemetry packet sim_latency ms after it was sent (components/gyminterface.py:96); with the fixed tick that is a delay of
 *   L ticks, L = ceil(ms * loop_hz / 1000).  Per env e a delay L_e in [0, max_ticks], max_ticks <= 30.
 *   T: the number of env steps taken since the later of trs_set_latency and trs_load_track — both begin the history.  trs_reset, a d_reset byte,
 *   auto_reset and trs_set_pose do NOT: the reference's pipeline keeps delivering the old episode's packets after reset_car.
 *   After step T the truth record is R_T = (frame, depth frame if cfg.depth, x, y, z, speed, cte, seg_idx), exactly as trs_get_state shows it.
 *     observation of env e after step T = R_{T - L_e}[e]                          when T - L_e >= 1
 *                                       = all frame bytes 0, depth 0.0f, telemetry 0, index 0   otherwise (the constructor's state, gyminterface.py:56,60-64)
 *     arrived[e] = (T - L_e >= 1)
 *   which is the delay line of HipGymInterface (it returns R_{t-L} from tick L + 1 on).  Nothing else is delayed: state, frames, rewards, done and
 *   returns of every existing call are the truth, bit for bit, whatever the delays.
 *   Closed loop (trs_step_pilot): the controls of tick T + 1 are KerasPilot.step(observation after T) for envs with arrived[e], and (0, 0, 0) for the
 *   others (keras_pilot.py:46-47: no frame yet); the speed (every model type that reads it) and 'loc/segment' (full house) are the observation's.
 *   The observation handed out after step T stays intact while step T + 1 runs.  tests/test_latency_cpu.py checks the ring arithmetic against a deque;
 *   tests/test_latency_gpu.py checks observations against the oracle's records kept in a list.
 *
 * ---- tub image (JPEG) (trs_encode_jpeg; the img_k.jpg of a tub record, components/datastorage.py:78; HIP library only) ---------------------------
 *   One uint8[H][W][3] RGB frame -> one baseline JPEG file: quality q in 1..100 (default 75), 4:2:0, one interleaved scan, the standard's tables.
 *   Integer arithmetic only; >> is an arithmetic shift, / truncates.  The file is a function of the frame's bytes, H, W and q alone.
 *   Quantisation tables: the luminance and chrominance bases of the JPEG standard's Annex K;  scale = q < 50 ? 5000 / q : 200 - 2 q;
 *     entry = clamp((base * scale + 50) / 100, 1, 255).
 *   Colour, per pixel, FIX(x) = (int)(x * 65536 + 0.5):
 *     Y  = ( FIX(.299) R   + FIX(.587) G   + FIX(.114) B   + 32768) >> 16
 *     Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B     + (128 << 16) + 32767) >> 16
 *     Cr = ( FIX(.5) R     - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
 *   MCU = 16 x 16 pixels = blocks Y00 Y01 Y10 Y11 Cb Cr of 8 x 8 samples; ceil(H / 16) x ceil(W / 16) MCUs in raster order.
 *   Edges.  The Y plane is padded to multiples of 8 by replicating its last column and row.  A full-resolution chroma plane is padded to an even
 *     height and to the width 16 ceil(W / 16) by replicating its last row and column, then downsampled; the DOWNSAMPLED plane is padded to a
 *     multiple of 8 rows by replicating ITS last row.  A Y block of an MCU that lies wholly beyond the ceil(H / 8) block rows or the ceil(W / 8)
 *     block columns is a dummy block: all AC coefficients 0, and its quantised DC is the quantised DC of the block before it in the MCU.
 *   Downsampling 2 x 2: (a + b + c + d + bias) >> 2, bias = 1 in even output columns and 2 in odd ones.
 *   DCT of a block of samples - 128: the integer forward transform with 13 constant bits and 2 extra bits after the first pass,
 *     DESCALE(x, n) = (x + (1 << (n - 1))) >> n.  One pass over d0..d7:
 *       t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4
 *       t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *       rows (first):    o0 = (t10 + t11) << 2,  o4 = (t10 - t11) << 2,  n = 11;      columns (second): o0 = DESCALE(t10 + t11, 2),  o4 = DESCALE(t10 - t11, 2),  n = 15
 *       e = (t12 + t13) * 4433;  o2 = DESCALE(e + t13 * 6270, n);  o6 = DESCALE(e - t12 * 15137, n)
 *       z5 = (t4 + t5 + t6 + t7) * 9633;  z1 = -(t4 + t7) * 7373;  z2 = -(t5 + t6) * 20995;  z3 = -(t4 + t6) * 16069 + z5;  z4 = -(t5 + t7) * 3196 + z5
 *       o7 = DESCALE(t4 * 2446 + z1 + z3, n);  o5 = DESCALE(t5 * 16819 + z2 + z4, n);  o3 = DESCALE(t6 * 25172 + z2 + z3, n);  o1 = DESCALE(t7 * 12299 + z1 + z4, n)
 *     over the 8 rows, then over the 8 columns: the coefficients come out scaled by 8.
 *   Quantiser, coefficient c, table entry Q:  qv = Q << 3;  a = |c| + (qv >> 1);  v = a >= qv ? a / qv : 0, with the sign of c.
 *   Entropy coding: the four Huffman tables of Annex K (codes of one length count up in symbol order and double when the length grows).  Per block in
 *     zig-zag order: the DC difference to the previous block of the same component (0 before the first; over the whole scan, no restart intervals) as
 *     its size s = bits of |d| and s extra bits (d, or d - 1 when negative); per non-zero AC coefficient 0xF0 (ZRL) while the run of zeros before it
 *     exceeds 15, then (run << 4 | s) and the s extra bits; 0x00 (EOB) when the block ends in zeros.  Bits fill bytes from the most significant one; a
 *     byte 0x00 follows every byte 0xFF; the last partial byte is filled with 1-bits; then FF D9.
 *   Header, in this order: SOI | APP0 "JFIF" 1.01, units 0, density 1 x 1, no thumbnail | DQT table 0, DQT table 1 (two segments, 8-bit, zig-zag) |
 *     SOF0 precision 8, H, W, components (1, 0x22, table 0) (2, 0x11, table 1) (3, 0x11, table 1) | DHT DC0, AC0, DC1, AC1 (four segments) |
 *     SOS components (1, 0x00) (2, 0x11) (3, 0x11), then 0, 63, 0.  623 bytes.
 *   This is what Pillow (libjpeg) writes for Image.fromarray(frame).save(path, quality=q): tests/test_jpeg_cpu.py restates the paragraph in numpy and
 *   compares files byte for byte; csrc/trsim_jpeg_tables.hpp is the one place the library's host and kernel take the rules from.
 *
 * ---- tub image (JPEG), decoding (trs_decode_jpeg; what the reference's loaders read back, components/keras_train.py:33-57; HIP library only) ------
 *   One baseline JPEG file -> one uint8[H][W][3] RGB frame and a status.  Integer arithmetic only; >> is an arithmetic shift.
 *   Accepted files: SOI; any APPn / COM segments (skipped); DQT and DHT taken FROM THE FILE (any number of 8-bit quantisation tables per segment,
 *     any quality; up to two DC and two AC Huffman tables in one or several segments, so files written with optimised tables decode); SOF0 with
 *     precision 8 and components (1, 0x22) (2, 0x11) (3, 0x11); one interleaved scan of components 1, 2, 3 with Ss = 0, Se = 63, Ah/Al = 0.
 *   Status, decided segment by segment in file order:  4 (corrupt): no SOI, a byte other than 0xFF where a marker must stand, a segment that runs
 *     past the file's end, a marker without a segment (0x00, 0x01, RSTn, SOI, EOI) before the scan, a table index > 3, a DHT with more codes of a
 *     length than that length has or more than 256 symbols, a second SOF0, SOS before SOF0 or naming a table the file did not define, segment
 *     lengths that contradict their counts.  2 (unsupported): fill bytes (0xFF 0xFF), 16-bit quantisation tables, Huffman table 2 or 3, APP14
 *     "Adobe", any other precision, component count, ids or sampling, any other frame type (SOF1..SOF15), DRI, any other scan parameters, any
 *     other marker, and a width <= 4 (a chroma plane <= 2 samples wide: libjpeg-turbo leaves the triangle filter there).  3: at SOS, H x W is not
 *     the expected size.  Then the scan: 4 when a bit at or beyond the end of the file is needed, when the next bits are no code of the table, when
 *     a marker (0xFF followed by anything but 0x00) stands before the last MCU is complete, when a DC size exceeds 11 or an AC size 10, or when a
 *     run leaves the block.  Otherwise 0; what follows the last MCU (padding, EOI) is not looked at.
 *   Entropy decoding is the inverse of the paragraph above: DC predictors per component over the whole scan, ZRL (16 zeros) and EOB, a 0x00 behind
 *     a 0xFF dropped; an extra-bits value v of size s stands for v if v >= 1 << (s - 1), else v - (1 << s) + 1.
 *   Dequantiser: coefficient k (zig-zag) times Q[k] of the component's table.
 *   Inverse DCT: 13 constant bits, 2 extra bits after the first pass, COLUMNS FIRST.  One pass over i0..i7:
 *       z1 = (i2 + i6) * 4433;  t2 = z1 - i6 * 15137;  t3 = z1 + i2 * 6270;  t0 = (i0 + i4) << 13;  t1 = (i0 - i4) << 13
 *       t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *       a0 = i7, a1 = i5, a2 = i3, a3 = i1;  z1 = a0 + a3, z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3, z5 = (z3 + z4) * 9633
 *       a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299;  z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5
 *       a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4
 *       o0..o7 = DESCALE(t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3; n)
 *     with n = 11 over the 8 columns, then n = 18 over the 8 rows; sample = clamp(o + 128, 0, 255).  (libjpeg's range table wraps for coefficients
 *     far outside what an image produces; that is not part of this paragraph: the arithmetic here wraps modulo 2^32 and then clamps.)
 *   Chroma upsampling: the 2 x 2 triangle filter over the ceil(H / 2) x ceil(W / 2) REAL samples of a chroma plane (the padding rows and columns
 *     the transform also produced are not read).  Image row y has the chroma row c = y >> 1 and the neighbour nb = the row above c when y is even,
 *     the row below when y is odd; above the first row and below the last stands that row itself.  s = 3 c + nb per chroma column.  Image column x
 *     has s of column x >> 1 and s' of the column to its left (x even) or right (x odd), which is that column itself at the plane's two ends:
 *     even x: (3 s + s' + 8) >> 4,  odd x: (3 s + s' + 7) >> 4.
 *   Colour, with cb, cr minus 128 and every result clamped to 0..255:
 *     R = Y + ((FIX(1.402) cr + 32768) >> 16);  G = Y + ((-FIX(0.34414) cb + 32768 - FIX(0.71414) cr) >> 16);  B = Y + ((FIX(1.772) cb + 32768) >> 16)
 *   This is what Pillow 12 on libjpeg-turbo gives for np.asarray(Image.open(path)): tests/test_jpeg_decode_cpu.py restates the paragraph in numpy
 *   and compares frames byte for byte; csrc/trsim_jpeg_decode.hpp is the one place the library's kernel and the host test driver take the rules from.
 *
 * ---- camera codec (JPEG round trip) (trs_jpeg_roundtrip, trs_set_camera_codec; the decoded 'cam/img' of components/gyminterface.py:97-99; HIP library only)
 *   codec(frame, q) of one uint8[H][W][3] RGB frame, W > 4, q in 1..100: the frame "tub image (JPEG), decoding" gives for the file "tub image
 *   (JPEG)" defines for `frame` at quality q.  Entropy coding is lossless, so no file is made; step by step, each as the paragraph named defines it:
 *     colour, edges, 2 x 2 downsampling, forward DCT (rows, then columns), quantiser                 ("tub image (JPEG)")
 *     dequantiser, inverse DCT (columns, then rows), clamp, triangle upsampling, colour              ("tub image (JPEG), decoding")
 *   The quantised coefficient v goes straight to the dequantiser: v times the table entry Q it was quantised with.
 *   Dummy Y blocks are never output: they hold no image sample, and what the file carries in them (the DC of the block before) does not reach a pixel.
 *   The padding rows and columns of the chroma planes take part in their blocks' transforms and are not read by the upsampler.
 *   The result equals what Pillow gives for save(quality = q), then open.  Parity with the closed simulator's own encoder is unpinned: its quality
 *   is unknown.  tests/test_jpeg_codec_cpu.py restates the paragraph in numpy and compares it with decode(encode()) of the two paragraphs above and with
 *   Pillow, byte for byte; csrc/trsim_jpeg_codec.hpp composes the two headers' rules for the kernel and for the host test driver.
 *
 * ---- scripted expert (trs_set_expert, trs_expert_act, trs_step_expert; the stand-in for the reference's human driver, components/controller.py:24; HIP library only)
 *   A rule on the env's own state (the truth of trs_state_view, never a delayed observation).  Every operation rounds to binary32 once (R1: no
 *   contraction, no fma), so a numpy float32 restatement is bit-exact.  Host, binary64, from the binary32 tangents of TRS_F_TANGENT:
 *     track_yaw[p] = (float)atan2((double)tx[p], (double)tz[p])
 *   profile: float[n_points], absent = +inf everywhere;  target: float[n_envs], absent = target_speed for every env.
 *   per env e:
 *     j      = (seg_idx + look) mod n_points                          look in [0, n_points)
 *     herr   = yaw - track_yaw[j];  if herr > PI: herr -= TWO_PI;  if herr < -PI: herr += TWO_PI
 *     steer  = clamp(-(k_cte*cte + k_head*herr), -1, 1)               (two products, one sum, one negation)
 *     v_ref  = min(target[e], profile[j])
 *     thr    = speed < v_ref ? thr_hi : thr_lo                        (strict <)
 *     brk    = speed > v_ref*brake_over ? brake_val : 0
 *   (steer, thr, brk) is the LABEL.  Disturbance, only in the closed loop of trs_step_expert, tick counter k since trs_set_expert:
 *     z  = SplitMix64 as in the synthetic control generator below, seed = the expert's seed, key = (global env id << 32) | k
 *     u  = (float)(z >> 40) * 2^-24
 *     w  = w + alpha*(sigma*(u*2 - 1) - w)
 *     applied_steer = clamp(steer + w, -1, 1);  throttle and brake are applied as labelled
 *   With sigma == 0, w stays 0 and the applied steering is the label.  w and k belong to the driver: resets of the car do not touch them,
 *   trs_set_expert zeroes them.  A record row is (steer, thr, brk, applied_steer, speed, cte, (float)((double)seg_idx / n_points * 10), done).
 *   tests/test_expert_cpu.py restates the paragraph in numpy and drives the CPU oracle with it; tests/test_expert_gpu.py compares the kernel with that
 *   restatement bit for bit; csrc/trsim_expert.hpp holds the host side (config checks, track_yaw, which ticks are captured).
 *
 * ---- pilot in the loop with the expert's labels (trs_step_dagger, trs_dagger_stats; dataset aggregation, DAgger; HIP library only) ----------------------
 *   The pilot drives, or a keyed mixture of pilot and expert; the expert's answer to every visited state is the label.  Binary32, one rounding per
 *   operation, no contraction, so a numpy float32 restatement is bit-exact.  Per tick, with the driver's counter k of "scripted expert" (zeroed by
 *   trs_set_expert, shared with trs_step_expert), per env e with global id gid = env_id_base + e:
 *     (ps, pt, pb) = the controls trs_step_pilot would apply this tick: KerasPilot.step on the same frame source (the latest frame; the delayed one under
 *                    "observation latency"; codec(that frame) under "camera codec"), the same speed, segment and mode mask; (0, 0, 0) before a frame exists
 *     (es, et, eb) = the LABEL of "scripted expert" on the truth.  The disturbance state w does NOT move and sigma is ignored (trs_step_expert moves it).
 *     z  = SplitMix64 as in the expert's disturbance, seed = trs_dagger_config.seed, key = (gid << 32) | (k / hold)      (integer division, hold >= 1)
 *     u  = (float)(z >> 40) * 2^-24
 *     expert drives = (u < beta)           beta = 0: never;  beta = 1: always, since u <= 1 - 2^-24.  Constant over blocks of `hold` ticks, keyed by
 *                                          the global env id: identical in every shard
 *     applied steering = expert drives ? es : ps
 *     expert_speed = 1 (default):  applied throttle, brake = (et, eb) always — "applied as labelled", as in trs_step_expert; the speed label of the
 *                                  speed_ctl and full_house loaders (the car's own speed / 20) then shows the expert's speed behaviour
 *     expert_speed = 0:            applied throttle, brake = expert drives ? (et, eb) : (pt, pb); those two loaders' speed label is then the PILOT's own
 *                                  speed and is not a correction
 *     row   = (es, et, eb, applied steering, speed, cte, (float)((double)seg_idx / n_points * 10), done), the layout of "scripted expert": the
 *             expert's label (TRS_LABEL_EXPERT) is the correction, the applied steering (TRS_LABEL_APPLIED) what the car was given
 *     frame = the frame the pilot was fed this tick: the codec's output under a camera codec, the delayed frame under a latency (zeros for the cars
 *             nothing has reached yet, as delivered), otherwise the latest frame.  This DIFFERS from trs_step_expert, which captures the rendered truth: it
 *             is the pair the pilot is judged on, and the pair the reference's tubs hold under sim_latency.
 *     stats[e], float[6], on every tick whether captured or not, in tick order, each one binary32 operation:
 *             [0] += 1;  [1] += expert drives ? 1 : 0;  [2] += |cte|;  [3] = max([3], |cte|);  [4] += |ps - es|;  [5] += done ? 1 : 0
 *             with cte and done of the state the label was computed on (the row's).  Counts are exact below 2^24 ticks.  Zeroed by trs_set_expert and by
 *             a reset request of trs_dagger_stats.
 *     k advances by one per tick.  Resets of a car touch neither k nor the stats.  The capture rule (which k is captured, into which slot) is
 *     trs_step_expert's; a tick whose frame is wanted is not captured while the pilot has no frame.
 *   tests/test_dagger_cpu.py restates the paragraph in numpy and drives the CPU oracle with it; tests/test_dagger_gpu.py compares trs_step_dagger with
 *   compositions of the existing calls and that restatement bit for bit; csrc/trsim_expert.hpp holds the defaults, the config check and the gate that the
 *   kernel and the host both use.
 *
 * ---- training minibatches (trs_sample_batch, trs_loader_order;DataLoader.load of the reference, components/keras_train.py:33-69; HIP library only)
 *   A set of n records (frame uint8[H][W][3], row float[8] as "scripted expert" defines it) stays where it is; a minibatch is gathered from it in a
 *   keyed order.  Everything below is unsigned 64-bit integer arithmetic (mod 2^64) or one IEEE operation, so a numpy restatement is bit-exact.
 *     mix(x):  z = x + 0x9E3779B97F4A7C15;  then the three finaliser lines of the synthetic control generator below
 *              (z ^= z>>30; z *= 0xBF58476D1CE4E5B9;  z ^= z>>27; z *= 0x94D049BB133111EB;  z ^= z>>31)
 *   perm(key, n, i), a bijection of [0, n) for n >= 1, computed per index without memory: a balanced Feistel network, cycle-walked.
 *     b = max(2, bit_length(n - 1)), rounded up to even;  h = b / 2;  mask = 2^h - 1;  x = i
 *     repeat:  L = x >> h;  R = x & mask
 *              for r = 0, 1, 2, 3:  (L, R) = (R, L ^ (mix(key ^ ((r << 32) | R)) & mask))
 *              x = (L << h) | R
 *     until x < n;  perm = x                         (2^b < 4n for n >= 2: the walk is short; it ends because the network permutes [0, 2^b))
 *   Split.  K = mix(seed);  sigma(i) = perm(K, n, i).  Split 0 (training) is sigma(0 .. n_train - 1), split 1 (validation) is
 *     sigma(n_train .. n - 1): off_0 = 0, n_0 = n_train, off_1 = n_train, n_1 = n - n_train.  n_train is given (Python: floor(split * n) in binary64,
 *     what sklearn's train_test_split computes for train_size = split).
 *   Epoch order.  K_e,s = mix(K ^ (((s + 1) << 32) | e)), e >= 0 the epoch, s the split.  Position p of epoch e of split s holds record
 *     sigma(off_s + perm(K_e,s, n_s, p)):  the same (seed, n, n_train, e, s, p) names the same record on every box and in every shard.
 *   Frames.  Per byte v of the record's frame: float32 (float)v / 255.0f (the one IEEE division of trs_normalize_kernel); binary16: that binary32 value
 *     rounded to nearest even; uint8: v.  Layouts NHWC [B][H][W][3] (the frame's own order) and, for float32 and binary16, NCHW [B][3][H][W].
 *   Features and labels of a row, as recorder.LOADERS gives them.  steer = row[0] (label "expert") or row[3] ("applied");
 *     s20 = (float)((double)row[4] / 20.0)   (the same bits as the one binary32 division row[4] / 20.0f: 53 >= 2 * 24 + 2)
 *       loader          features            labels
 *       speed_ctl       -                   (steer, s20)
 *       default         -                   (steer, row[1])
 *       speed_feature   (s20)               (steer, row[1])
 *       full_house      (s20, row[6])       (steer, s20)
 *   tests/test_loader_cpu.py restates the paragraph in numpy and compares trs_loader_order with it; tests/test_loader_gpu.py compares trs_batch_kernel
 *   with that restatement bit for bit; csrc/trsim_loader.hpp is the one place the kernel and the host take the rules from.
 *
 * ---- training minibatches, augmentation (trs_sample_batch_aug, trs_loader_augment; HIP library only)
 *   A record of a minibatch is mirrored left to right and lit again, by draws that are a function of (aug.seed, epoch, record number) alone: not of the
 *   batch slot, the batch size, `first` or the split the record sits in.  Unsigned 64-bit arithmetic (mod 2^64) and single binary32 IEEE operations only;
 *   mix is the function of "training minibatches".
 *     A        = mix(aug.seed ^ 0x6175676D656E7421)
 *     k(e, r)  = mix(A ^ (((uint64)e << 32) | r))           e >= 0 the epoch, r the record number (what d_index reports)
 *     d_j      = mix(k + j) >> 40                            j = 0 .. 6, 24 bits each
 *     mirror   = d_0 < T,  T = (uint32)((double)mirror_prob * 16777216.0)       (mirror_prob 1: always; 0: never)
 *     f_j      = (float)d_j * 0x1p-23f - 1.0f                exact, in [-1, 1)
 *     gain_c   = 1.0f + f_(1+c) * gain_amp                   two roundings: the product, then the sum (no fused multiply-add)
 *     bias_c   = f_(4+c) * bias_amp                          c = 0, 1, 2 = R, G, B
 *     per_channel == 0:  gain_c = gain_0 and bias_c = bias_0 for every c (draws j = 1 and j = 4 only)
 *   Pixel.   Every byte x of channel c of the record's frame becomes light_channel(x, gain_c, bias_c) first: rule R1 of "scene lighting", verbatim, the
 *            one shared function.  The conversion of "training minibatches" (float32, binary16 or the byte) follows.
 *   Mirror.  On a mirrored record, for every channel, out[y][x] = lit[y][W - 1 - x].  (The class map is a function of the distance to the centre line
 *            and the arc length, and the pinhole camera has no roll: the mirror image of a frame is the frame of the mirrored track.)
 *   Label.   On a mirrored record label[0] (whichever steering cfg.label selects) has its sign bit flipped: 0.0f becomes -0.0f.
 *   label[1], the features, d_index and the order are unchanged; a physics-only set gets the label rule alone.
 *   Refused: mirror_prob outside [0, 1], gain_amp outside [0, 1) (the gain stays positive), bias_amp outside [0, 255] (a NaN is outside),
 *   per_channel not 0 or 1, mirror_prob > 0 with the full_house loader (row[6] is a position on the track as driven).
 *   Off (mirror_prob == 0, gain_amp == 0, bias_amp == 0, or no config): trs_sample_batch itself.
 *   Test vectors, seed 0, epoch 0, record 0:  d_0..6 = 11521308 2773027 14270921 1147758 4524845 10059823 8999555;  mirror_prob 0.5: not mirrored;
 *     gain_amp 0.25: gains 3f552812 3f967072 3f48c1b7;  bias_amp 32: biases c16bd34c 40cc0178 40152830 (bit patterns).
 *     Mirror flags of records 0..11 at mirror_prob 0.5, seed 0:  epoch 0: 0 1 1 0 0 0 0 0 0 1 1 0;  epoch 1: 1 0 1 0 0 1 1 0 1 0 0 0.
 *     Mirrored among records 0..4095 at 0.5, epochs 0, 1, 7:  seed 0: 2068 1996 2052;  seed 1: 2081 2042 2019;  seed 12345: 1984 2068 2001.
 *   tests/test_augment_cpu.py restates the paragraph in numpy and compares trs_loader_augment with it; tests/test_augment_gpu.py compares
 *   trs_batch_aug_kernel with that restatement bit for bit; csrc/trsim_augment.hpp is the one place the kernel and the host take the draw from.
 *
 * ---- training the pilot's tail (trs_pilot_train_begin, trs_pilot_train_step; 22-array model types; HIP library only)
 *   dense1 -> dense2 -> dense3 -> output_layer of the loaded pilot move by Adam on Keras's 'mse' (components/keras_train.py:400-404); conv1 .. conv7 stay as
 *   loaded.  Inputs of a step: n frames uint8 NHWC, labels y[n][2] binary32, 1 <= n <= n_envs.  W(l), b(l): kernel [IN][OUT] and bias of layer l = 1..4.
 *   1. Forward, by the kernels that drive: conv1 .. conv7 and trs_pilot_dense_kernel with the current binary16 copy of W1.  Per frame z1 = the split-K slabs
 *      added in slice order (binary32, from +0), a1 = relu(z1); z2, z3 and out are one fmaf chain per output from the bias with k ascending,
 *      s = fmaf(a[k], W[k][o], s), a = relu(z) in between.  out equals trs_pilot_forward's on the same frames bit for bit.
 *   2. loss = sum_i sum_j (out_ij - y_ij)^2 / (2 n): binary32, s = fmaf(e, e, s) over i ascending, j ascending inside, then one division by (float)(2 n).
 *      delta4_ij = (out_ij - y_ij) / (float)n: a subtraction and a correctly rounded division.
 *   3. Backward in binary32, per frame: delta(l)[k] = [z(l)[k] > 0] * sum_o W(l+1)[k][o] delta(l+1)[o] for l = 3, 2, 1; the sum is one fmaf chain from +0 with
 *      o ascending, s = fmaf(W[k][o], delta[o], s).
 *   4. Small gradients in binary32, one chain per value over the frames in ascending order: gW(l)[k][o] = sum_i a(l-1)_i[k] delta(l)_i[o] for l = 2, 3, 4 as
 *      s = fmaf(a, delta, s) from +0; gb(l)[o] = sum_i delta(l)_i[o] for l = 1..4 as s = s + delta.  No floating-point atomics anywhere.
 *   5. gW1[k][o] = sum_i x7_i[k] delta1_i[o], x7 = conv7's binary16 activation as stored, on the matrix cores with delta1 as binary16 under a power-of-two
 *      scale per batch.  B = the integer maximum over the batch of the bit patterns of |delta1| (equal to the pattern of the largest value).
 *        B == 0:                 s = 0
 *        exponent field of B 0:  E = (position of B's leading one) - 149          (a subnormal)
 *        otherwise:              E = (B >> 23) - 127                               (Inf and NaN patterns: 128)
 *        s = 14 - E clamped to [-100, 100];  q = binary16_rn(delta1 * 2^s)  (the product exact in binary32, one rounding to nearest even; the largest
 *        value lands in [2^14, 2^15));  gW1 = 2^-s * sum_i x7 q, the products exact and the sum accumulated in binary32 by the MFMA, the frames of a k-step of
 *        16 in the hardware's order, the k-steps ascending; one workgroup owns a feature for the whole batch.  The last factor is one binary32 multiply.
 *   6. Adam in Keras's form, t counting the steps from 1.  Constants: b1 = beta1, b2 = beta2, e = eps as binary32; c1 = (float)(1 - (double)b1),
 *      c2 = (float)(1 - (double)b2); alpha_t = (float)((double)lr * sqrt(1 - (double)b2^t) / (1 - (double)b1^t)) (binary64 sqrt and pow, one rounding).
 *      Per value, plain binary32, every operation rounded by itself, no contraction, sqrt and / correctly rounded:
 *        m = (b1 * m) + (c1 * g)
 *        v = (b2 * v) + (c2 * (g * g))
 *        w = w - ((alpha_t * m) / (sqrt(v) + e))
 *      on fp32 masters (trs_pilot_train_begin: W1 from the caller's array, the rest from the device), m = v = 0 at the start.  The pass over W1 also writes
 *      its binary16 granules [G][128][8] with host_f2h's rounding (nearest even, 65504 beyond the range); the other seven arrays are also written where the
 *      tail kernels read them.  A layer whose bit of train_mask is clear keeps w, m and v; t counts all the same.
 *   Vectors.  Exponent: B = 0 -> 0; 1.0f -> 14; 1.9999999f -> 14; 2.0f -> 13; 0.5f -> 15; 3e-6f -> 33; 2^14 -> 0; 2^15 -> -1; 2^-86, 2^-87 -> 100;
 *     B = 1, 0x00400000, 0x007FFFFF -> 100; 2^114, 2^120, 0x7F800000, 0x7FC00000 -> -100.
 *     alpha_t at the defaults (bit patterns): t = 1: 39a5cb17, t = 2: 3976beef, t = 1000: 3a507326.  c1 = 3dccccd0, c2 = 3a831200.
 *     One update, g = 1, m = v = 0, w = 1, t = 1: m = 3dccccd0, v = 3a831200, w = 3f7fbe77 (0.99900001: Adam's first step is lr in size).
 *   Not here: conv1 .. conv3 (conv4 .. conv7: the next section), dropout behind conv1 .. conv6 (behind conv7 and the hidden dense layers: "training the
 *   pilot's tail, dropout"; keras_train.py applies 0.1 everywhere; tests/golden/train_pilot_fixture.py trains without), cnn_2d_full_house (42 arrays:
 *   refused; the 28-array type: "training the pilot's tail, side branch"), feature caching across epochs, gradient exchange between GPUs.
 *   tests/test_train_cpu.py restates steps 2 to 6 in numpy and checks the restatement against torch.autograd in binary64; tests/test_train_gpu.py compares the
 *   kernels with it (Adam bit for bit from the device's gradient); csrc/trsim_train.hpp holds the rules a host compiler can build.
 *
 * ---- training the pilot's last convolutions (trs_pilot_train_convs; conv4 .. conv7 of a 22-array model type; HIP library only)
 *   After trs_pilot_train_convs(mask) a step of the tail's session also moves the layers l of conv4 .. conv7 whose bit l - 4 is set; all four are 3 x 3,
 *   stride 1, valid, (CIN, COUT) = (64, 64), (64, 64), (64, 128), (128, 128).  x(l) = conv_l's stored binary16 activation [n][OH][OW][COUT], W(l)h = its
 *   binary16 kernel as the forward kernels read it, lo = the lowest layer named.  Without the call a step is the tail's section, bit for bit.
 *   1. Forward: unchanged, by the kernels that drive; out of a step equals trs_pilot_forward bit for bit.  x3 and x7 are as the pass stored them; x4 .. x6 are
 *      what the single-layer kernels compute from x3 where the fused chain kept them in LDS (materialise_layers), before any weight moves.  At 96x128 and
 *      120x160 the single-layer conv7 on the materialised x6 reproduces the chain's x7 bit for bit (tests/test_train_conv_gpu.py).
 *   2. G7_i[k] = [x7_i[k] > 0] * 2^-s * sum_o W1h[k][o] q1_i[o], k over the flatten: on the matrix cores from the binary16 dense1 copy the forward used (before
 *      the tail's Adam rewrites it) and the q1 and s of the tail's step 5.  The products are exact in binary32; the 128 outputs (100 and zero padding) are
 *      added in the MFMA's order, k-steps of 16 ascending; one binary32 multiply by 2^-s.
 *   3. delta(l) is G(l) stored as binary16 under a per-layer, per-batch scale: B_l = the integer maximum (atomicMax) of the bit patterns of |G(l)|,
 *      s_l = the tail's exponent rule on B_l (train_scale_exponent), q(l) = binary16_rn(G(l) * 2^s_l), delta(l) = q(l) * 2^-s_l.
 *   4. For l = 7 .. lo + 1: G(l-1)[f][y][x][ci] = [x(l-1) > 0] * 2^-s_l * sum_{kh,kw,co} q(l)[f][y-kh][x-kw][co] * W(l)h[kh][kw][ci][co], terms outside q's
 *      extent zero.  Matrix cores, binary32 accumulator, the sum in the order kh, kw ascending, inside a tap the k-steps of 16 co ascending.  Nothing is
 *      computed below x(lo - 1): in particular nothing for x3.
 *   5. For every trained l: gW(l)[kh][kw][ci][co] = 2^-s_l * sum_{f,oy,ox} x(l-1)[f][oy+kh][ox+kw][ci] * q(l)[f][oy][ox][co] on the matrix cores, binary32.
 *      The P = n OH OW output pixels in (f, oy, ox) order are cut into chunks of 64; with want = max(1, min(chunks, (2 CUs + 8) / 9)),
 *      per_slice = ceil(chunks / want) and slices = ceil(chunks / per_slice), slice s takes chunks s per_slice .. (a function of the geometry, n and the CU
 *      count alone).  One workgroup per (slice, tap) adds its chunks in order (k-steps of 16 pixels ascending); the slices' sums are added in slice order,
 *      then one multiply by 2^-s_l.  gb(l)[co] = 2^-s_l * sum q(l)[.][co]: per slice and channel, 256 / COUT running sums over the pixels p with equal
 *      p mod (256 / COUT), added in that order, then the slices in slice order.  No floating-point atomics anywhere: two runs agree bit for bit.
 *   6. Adam: the tail's step 6 verbatim, the same alpha_t and t, on fp32 masters of the trained kernels and biases (from the arrays given to
 *      trs_pilot_train_convs), m = v = 0 at the start.  The pass writes each kernel's binary16 value with host_f2h's rounding at
 *      ((kh run_pad + kw CIN / 8 + ci / 8) COUT_PAD + co) 8 + ci % 8 of ConvLayer::w (pack_layer's order; run_pad = 3 CIN / 8, COUT_PAD = COUT), into the
 *      session's own [kh][kw][ci][co] copy that step 4 reads, and the bias where the kernels read it.  Step 4 of layer l runs before layer l's Adam.
 *   Not here: conv1 .. conv3 (5 x 5, stride 2, the fused head), dropout behind conv1 .. conv6, the 42-array model type, feature caching, the
 *   multi-GPU exchange.
 *   tests/test_train_conv_cpu.py restates steps 2 to 5 in numpy, checks the restatement against torch.autograd in binary64 and shows what the reference
 *   notices; tests/test_train_conv_gpu.py compares the kernels with it within derived bounds (Adam bit for bit from the device's gradient);
 *   csrc/trsim_train_conv.hpp holds the rules a host compiler can build (tests/train_conv_driver.cpp).
 *
 * ---- training the pilot's tail, dropout (trs_pilot_train_dropout, trs_train_dropout_keep; HIP library only)
 *   The reference's trainer puts Dropout(0.1) behind every convolution and every hidden dense layer (components/keras_train.py:131-164).  After
 *   trs_pilot_train_dropout(rate, sites, seed) the steps of a session drop at the four sites the session owns: site 0 (bit 1 of sites) conv7's output x7,
 *   the flatten dense1 reads, F units per frame; sites 1, 2, 3 (bits 2, 4, 8) relu(z1), relu(z2), relu(z3): 100, 50, 25 units per frame.  The sites behind
 *   conv1 .. conv6 stay out: they lie inside forward kernels that also drive, and those kernels do not change.  Inference never drops: trs_pilot_forward,
 *   trs_pilot_act, trs_step_pilot, trs_step_dagger and pilot_loss are untouched, as in Keras.  Unsigned 64-bit arithmetic (mod 2^64) and single binary32
 *   IEEE operations only; mix is the function of "training minibatches".
 *     T     = floor((double)rate * 65536)                    rate a binary32 in [0, 1): 0 <= T <= 65535; the effective rate is T / 65536
 *     s     = (float)(65536.0 / (65536 - T))                 the scale of the EFFECTIVE rate: s (1 - T / 65536) = 1 to one rounding
 *     D     = mix(seed ^ 0x64726F706F757421)
 *     Dt    = mix(D ^ t)                                     t >= 1: the session's step count, the t of alpha_t
 *     key   = mix(Dt ^ (((uint64)site << 32) | i))           i: the frame's slot in the batch
 *     word  = mix(key + (k >> 2)),  field = (word >> (16 (k & 3))) & 0xFFFF       unit k of the frame: four units per mix
 *     keep  = field >= T
 *   The flags are a function of (seed, t, site, i, k) alone: a batch of 70 has the batch of 17 as its prefix.
 *   Forward.  Sites 1 .. 3: a'(l)[k] = keep ? relu(z(l)[k]) * s : +0, one binary32 rounding; a'(l) replaces relu(z(l)) as the next layer's input (step 1 of
 *     "training the pilot's tail") and in the weight gradient of layer l + 1 (step 4).  Site 0: x7'[f] = keep ? binary16_rn(min((float)x7[f] * s, 65504)) :
 *     +0, written where dense1 and the gW1 GEMM (step 5) read x7, before dense1 runs (x7 is finite and not negative: a ReLU's output).  out, the loss
 *     and every gradient of a step are those of the dropped network.
 *   Backward.  delta(l) = ((W(l+1) delta(l+1)) * s) . keep . [z(l) > 0] for l = 3, 2, 1: the chain of step 3, then one more binary32 product.  With
 *     trs_pilot_train_convs, G7 = [x7' > 0] . (s * 2^-s1) (W1h q1): the gate on the dropped x7' carries the mask (a kept positive value stays positive, s >= 1),
 *     and s * 2^-s1 is one binary32 product, exact, since one factor is a power of two.  Nothing else of the convolutions' backward pass changes: x7 is only a
 *     gate there.
 *   Off.  No call, rate 0 (T = 0) or a clear site bit: that site computes what the two sections above state, bit for bit, by the same kernels.
 *   Refused: a struct_size mismatch, a rate that is NaN or outside [0, 1), sites with bits above 3 (TRS_ERR_ARG); the call without a session, after the
 *   session's first step, or twice (TRS_ERR_STATE).
 *   Vectors.  rate 0.1f: T = 6553, s = 3f8e3885;  0.5f: T = 32768, s = 2;  0.999f: T = 65470;  the largest binary32 below 1: T = 65535, s = 65536.
 *     Kept among the 70 x 4608 units of site 0 at rate 0.1f, seed 0, t = 1: 290315 (0.900034 against 1 - T / 65536 = 0.900009).
 *   tests/test_dropout_cpu.py restates the paragraph in numpy, compares trs_train_dropout_keep with it bit for bit and checks the dropped passes against
 *   torch.autograd in binary64 with the masks as constants; tests/test_dropout_gpu.py compares the kernels with it (x7' and a'(l) bit for bit);
 *   csrc/trsim_dropout.hpp is the one place the kernels and the host take the draw from (tests/dropout_driver.cpp).
 *
 * ---- training the pilot's tail, side branch (trs_pilot_train_begin_ex, trs_pilot_train_step_ex; the 28-array model type; HIP library only)
 *   cnn_2d_speed_as_feature = Keras_2D_CNN.get_model(num_feature_vectors = 1) (components/keras_train.py:127-174,390-392): the car's speed / 20 goes through
 *   feature1 -> feature2 -> feature3 (Dense 4, 8, 16, ReLU) and is concatenated behind the flatten in front of dense1.  The session trains 14 arrays, arrays
 *   14 .. 27 of trs_pilot_load: dense1 .. output_layer as in "training the pilot's tail", with W1 of (F + 16) x 100 values, then F1, bF1, F2, bF2, F3, bF3
 *   (kernels [IN][OUT]).  W1Y = rows F .. F + 15 of W1, kept in binary32 where trs_pilot_tail_ex_kernel reads them; rows 0 .. F - 1 are the flatten's, as before.
 *   Inputs of a step: the frames and labels of the tail's section and s20[n][1] binary32, the feature as the speed_feature loader delivers it
 *   (s20 = row[4] / 20: the same bits as the speed / 20.0f trs_pilot_tail_ex_kernel computes).
 *   1. Forward.  fin = s20.  y1[j] = relu(fmaf(fin, F1[0][j], bF1[j])), 4 values; y2 = relu(F2^T y1 + bF2), 8 values, and y3 = relu(F3^T y2 + bF3), 16
 *      values: one fmaf chain per unit from the bias, k ascending, s = fmaf(y[k], F[k][o], s) — what dense_small computes.  z1 = the split-K slabs added in
 *      slice order (binary32, from +0), then z1 = fmaf(y3[k], W1Y[k][o], z1) for k = 0 .. 15 ascending.  a1 = relu(z1), and dense2 -> dense3 -> output_layer
 *      follow as in step 1 of the tail's section.  out equals trs_pilot_forward_ex's on the same frames and speeds bit for bit.
 *   2. The loss and delta4 .. delta1: steps 2 and 3 of the tail's section, unchanged.
 *   3. Through the branch, binary32, per frame: delta-y3[k] = [y3[k] > 0] * sum_o W1Y[k][o] delta1[o], o = 0 .. 99 ascending; delta-y2[j] = [y2[j] > 0] *
 *      sum_k F3[j][k] delta-y3[k]; delta-y1[j] = [y1[j] > 0] * sum_k F2[j][k] delta-y2[k]: each one fmaf chain from +0, s = fmaf(W[row][o], delta[o], s).
 *   4. Gradients, binary32, one chain per value over the frames in ascending order, as step 4 of the tail's section: gW1Y[k][o] = sum_i y3_i[k] delta1_i[o],
 *      gF3[j][k] = sum_i y2_i[j] delta-y3_i[k], gF2[j][k] = sum_i y1_i[j] delta-y2_i[k] as s = fmaf(y, delta, s) from +0; gbF3, gbF2, gbF1 = sum_i of
 *      delta-y3, delta-y2, delta-y1 as s = s + delta.  gF1[0][j] = sum_i p_i[j] with p_i[j] = fin_i * delta-y1_i[j], one binary32 product, as s = s + p: the
 *      feature may be negative, and the chains of the first form gate their first factor.  The rows 0 .. F - 1 of gW1 are step 5 of the tail's section over
 *      x7 and the quantised delta1: the matrix-core GEMM does not see the branch.
 *   5. Adam: step 6 of the tail's section over all 14 arrays; W1Y and the six branch arrays are also written where trs_pilot_tail_ex_kernel reads them, so
 *      the handle drives with the updated pilot.  Bits 0 .. 3 of train_mask are the tail's layers (W1Y moves with dense1), bits 4 .. 6 feature1 .. feature3.
 *   Dropout (the section above): site 0 masks x7 alone, since Keras concatenates behind the Dropout on x; sites 1 .. 3 are unchanged, and delta-y3 is taken
 *      from the delta1 that carries site 1's mask and scale.  The feature layers have no dropout in the reference: fin, y1 .. y3 are the same with and without.
 *   The convolutions (trs_pilot_train_convs): G7 reads q1, the binary16 copy of rows 0 .. F - 1 of W1 and x7 alone, so the section applies as it stands.
 *   No floating-point atomics anywhere: two runs agree bit for bit.
 *   Not here: cnn_2d_full_house (42 arrays: its two heads both feed conv7's gradient; refused with TRS_ERR_LIMIT), and what the tail's section leaves out.
 *   tests/test_train_side_cpu.py restates steps 1 to 4 in numpy and checks the restatement against torch.autograd in binary64; tests/test_train_side_gpu.py
 *   compares the kernels with it (out, fin, y1 .. y3 and Adam bit for bit); csrc/trsim_train.hpp holds the layout of the 14 arrays and the count and mask rules
 *   (tests/train_side_driver.cpp).
 */
#ifndef TRSIM_SPEC_H
#define TRSIM_SPEC_H

/* trig */
#define TRS_PI            3.14159274101257324f   /* (float)pi */
#define TRS_TWO_PI        6.28318548202514648f
#define TRS_TWO_OVER_PI   0.636619746685028076f
#define TRS_PIO2_HI       1.5707963705062866211f /* (float)(pi/2) */
#define TRS_PIO2_LO      -4.3711388286737928865e-08f /* (float)(pi/2 - PIO2_HI) */
#define TRS_S0           -1.9515295891e-4f
#define TRS_S1            8.3321608736e-3f
#define TRS_S2           -1.6666654611e-1f
#define TRS_C0            2.443315711809948e-5f
#define TRS_C1           -1.388731625493765e-3f
#define TRS_C2            4.166664568298827e-2f

/* default physics parameters (trs_config overrides) */
#define TRS_DEF_DT              0.05f          /* 20 Hz: car_templates/manage.py:38 */
#define TRS_DEF_MAX_STEER       0.43633231520652770996f /* 25 deg */
#define TRS_DEF_INV_WHEELBASE   0.8333333134651184082f /* 1/1.2 */
#define TRS_DEF_ACCEL_MAX       10.0f
#define TRS_DEF_DRAG_LIN        0.5f           /* terminal speed 20 = pilots' full scale, keras_pilot.py:83 */
#define TRS_DEF_ROLL_RES        0.3f
#define TRS_DEF_BRAKE_MAX       15.0f
#define TRS_DEF_V_MAX           25.0f
#define TRS_DEF_V_REV_MAX       5.0f
#define TRS_DEF_OFFTRACK_CTE    3.0f
#define TRS_DEF_OFFTRACK_PENALTY 10.0f
#define TRS_LOST_L1             100.0          /* track_data_process.py:93 */

/* default track-surface parameters (world units) */
#define TRS_DEF_ROAD_HALF       2.0
#define TRS_DEF_EDGE_HALF       0.10
#define TRS_DEF_CENTRE_HALF     0.075
#define TRS_DEF_DASH_PERIOD     3.0
#define TRS_DEF_DASH_ON         1.5
#define TRS_DEF_MAP_MARGIN      2.5            /* world units of class-0 border around the track bbox (>= road_half + edge_half + one cell;
                                                  lookups outside the map clamp to this grass border) */
#define TRS_NEAR_GRID_CELL      4.0            /* nearest-point accelerator: 3x3 block of cells of this size; exact by the rule below */
#define TRS_MAP_CELL_MIN        0.125          /* cell sizes are 0.125 * 2^k so 1/cell is exact */
#define TRS_MAP_LDS_BUDGET      (96 * 1024)    /* the packed 2-bit map must fit this many bytes */

/* default camera */
#define TRS_DEF_FOV_V_DEG       80.0           /* gyminterface.py:27 (unused there) */
#define TRS_DEF_CAM_H           1.0
#define TRS_DEF_CAM_PITCH_DEG   10.0
#define TRS_DEF_CAM_FWD         0.3f
#define TRS_DEF_Z_FAR           40.0

/* tracks with elevation */
#define TRS_HILL_MIN_RANGE      0.25           /* max y - min y of the raw points above which a track is hilly */
#define TRS_HILL_SPAN           8              /* grade over +- this many samples */
#define TRS_HILL_AHEAD          24             /* the slope this many samples ahead against the slope here */
#define TRS_HILL_MAX_DPITCH     0.2            /* rad */

/* map classes */
#define TRS_CLS_GRASS   0
#define TRS_CLS_ROAD    1
#define TRS_CLS_EDGE    2
#define TRS_CLS_CENTRE  3

/* base colours, RGB */
#define TRS_RGB_GRASS   { 58, 132,  62}
#define TRS_RGB_ROAD    { 92,  92,  98}
#define TRS_RGB_EDGE    {236, 236, 236}
#define TRS_RGB_CENTRE  {232, 200,  40}
#define TRS_RGB_FOG     {176, 196, 208}
#define TRS_RGB_SKY_TOP {104, 156, 228}
#define TRS_RGB_SKY_HOR {192, 216, 240}
#define TRS_FOG_MAX     0.65                   /* fog weight at z_far */

/* synthetic control generator: SplitMix64 keyed by (seed, global env id, step)
 *   z = seed + ((env_gid << 32) | step) * 0x9E3779B97F4A7C15;  z ^= z>>30; z *= 0xBF58476D1CE4E5B9;
 *   z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31
 *   us = (float)(z >> 40) * 2^-24;  ut = (float)((z >> 16) & 0xFFFFFF) * 2^-24
 *   steer_raw = us*2 - 1;  sf = sf + 0.1f*(steer_raw - sf);  steer = sf
 *   thr = 0.2f + 0.6f*ut;  brk = 0
 */
#define TRS_SYNTH_SEED      0x5EEDull
#define TRS_SYNTH_ALPHA     0.1f
#define TRS_SYNTH_THR_LO    0.2f
#define TRS_SYNTH_THR_SPAN  0.6f
#define TRS_START_STRIDE    37                 /* env i starts at track point (37*i) mod n */

/* scripted expert: defaults of trs_expert_config (trs_default_expert_config) */
#define TRS_EXPERT_LOOK         6
#define TRS_EXPERT_K_CTE        1.0f
#define TRS_EXPERT_K_HEAD       2.0f
#define TRS_EXPERT_THR_HI       0.6f
#define TRS_EXPERT_THR_LO       0.1f
#define TRS_EXPERT_TARGET_SPEED 6.0f
#define TRS_EXPERT_BRAKE_OVER   1.15f
#define TRS_EXPERT_BRAKE_VAL    0.5f
#define TRS_EXPERT_ALPHA        0.1f
#define TRS_EXPERT_SIGMA        0.0f
#define TRS_EXPERT_SEED         0ull           /* the fixture's (tests/golden/train_pilot_fixture.py: collect(seed=0)) */
/* pilot in the loop with the expert's labels: defaults of trs_dagger_config (trs_default_dagger_config) */
#define TRS_DAGGER_BETA         0.5f
#define TRS_DAGGER_HOLD         1
#define TRS_DAGGER_EXPERT_SPEED 1
#define TRS_DAGGER_SEED         0ull

#endif /* TRSIM_SPEC_H */
