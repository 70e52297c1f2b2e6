// ksw_row_step.inc -- one step of a strip in extd2_team_kernel: every lane of a team does ONE ROW of its CPL columns, left to right;
// lane ql is ql rows behind lane 0 (step k: row k - ql).  Included three times by ksw_kernels.hip: TEAM_MASKED 1 for the first
// LANES - 1 steps (a lane that has not started must keep its state), TEAM_MASKED 0 afterwards (what a lane computes past its last row
// is never looked at); TEAM_TOPROW 1 for the steps in which some lane is in row 0 (k < LANES).
		const int i = k - ql;                                           // this lane's row
		const bool act = (unsigned)i < (unsigned)qlen;
		// -- first, everything that looks at what the step before loaded (q_cur, e_prev, d_cur): the one wait of the step stands here.
		// The empty statement names the three as used, so the compiler waits for them here, at the top, whatever it sinks into the
		// branches below or into the cluster (left alone it waited behind the cluster's first store, for a register it reuses).
		asm volatile("" : "+v"(q_cur), "+v"(e_prev));
		if (!LEAN) asm volatile("" : "+v"(d_cur));
		const int qc4 = (int)((q_cur << 2) & 0x1cu);                    // the row's query code, times four: column offset in the score table
		// the column left of this lane's first one, same row: the neighbour lane's last column (it did this row one step ago), or for the
		// team's first lane column -1 (:142-152) / the previous strip's last column
		int vl = 0, xl = 0, x2l = 0;
		if (LANES > 1) {
			vl = __builtin_amdgcn_update_dpp(0, V[CPL - 1], 0x111, 0xf, 0xf, false), xl = __builtin_amdgcn_update_dpp(0, X[CPL - 1], 0x111, 0xf, 0xf, false);
			x2l = __builtin_amdgcn_update_dpp(0, X2[CPL - 1], 0x111, 0xf, 0xf, false);
			if (!LEAN) {
				// the anti-diagonal that left the neighbour on the right one step ago passes this lane's last but one column now
				const int inc = __builtin_amdgcn_update_dpp(kNone, out_prev, 0x101, 0xf, 0xf, false);
				M[CPL - 2] = max(M[CPL - 2], ql == LANES - 1 ? kNone : inc);
			}
		}
		// D of this step's diagonal as the strips before left it: they wrote it as far as their drain went (it ends at c0 + ksteps - LANES)
		const int d_row = (!LEAN && s > 0 && k <= ksteps - LANES) ? d_cur : kNone;
		if (ql == 0) {
			// the previous strip's last column, one dword: v / 8, (x - 3) / 8, (x2 - 1) / 8 as signed bytes (v is a multiple of 8, x and x2 are
			// multiples of 8 plus their constant priority tag, and the true differences fit int8 in this regime)
			if (s > 0) vl = __builtin_amdgcn_sbfe((int)e_prev, 0, 8) << 3, xl = (__builtin_amdgcn_sbfe((int)e_prev, 8, 8) << 3) | 3, x2l = (__builtin_amdgcn_sbfe((int)e_prev, 16, 8) << 3) | 1;
			else vl = 8 * ur_of(i), xl = x_init, x2l = x2_init;
		}
		// -- then the step's memory operations, as one cluster in straight-line code: what the step before left to store (its direction
		// bytes, its strip-boundary dword or last-column H) and the loads for the step after.  Nothing below looks at them, so they have
		// the whole step to complete.  The loads are unconditional: a row index past the query is clamped, Ein / uD rows that no strip
		// wrote lie inside the wavefront's scratch, and what they return is never looked at (act, s > 0, d_row above).
		__builtin_amdgcn_sched_barrier(0);
		if (with_cigar && (!TEAM_MASKED || k > 0)) {
			uint32_t *const dst = (uint32_t *)(w0 + (size_t)(s * R + k - 1) * (64 * CPL) + lc);
#pragma unroll
			for (int g = 0; g < CPL / 4; ++g) dst[g] = dirw[g];
		}
		if (CARRY) {
			// row i - 1, the one this lane did a step ago (none in step 0): a wave-uniform row base plus the lane's constant offset; the
			// lane's predicate and "that row was inside the query" are one compare (qlen_e / qlen_o are 0 in a lane that stores nothing)
			const long long rowb = (long long)(k - 1) * (4 * PB);
			if ((unsigned)(i - 1) < qlen_e) *(int *)(Eout + rowb + eoff) = (int)carry;
			if ((unsigned)(i - 1) < qlen_o) *(short *)(uD23 + rowb + ooff) = (short)carry;
		}
		q_cur = query[min(TEAM_MASKED ? max(i + 1, 0) : i + 1, qlen - 1)];   // (i + 1 >= 1 once every lane has started)
		e_prev = (unsigned)at4(Ein, k + 1);
		if (!LEAN) d_cur = at4(uD, c0 + k + 1);
		__builtin_amdgcn_sched_barrier(0);
		// The reference's order among equal H on an anti-diagonal (:322-349): whole 4-cell groups first, by (place & 3, place), then the
		// tail in place order; the cell at en0, which it looks at first, is settled afterwards.  place = t - st0 is the column itself while
		// the diagonal starts in row >= 0 of column 0 (t <= qlen - 1 - i) and qlen - 1 - i, the same for the whole row, below that; rank
		// bits of a place: frank().  "Not in the tail" (bit 14) is t < st0 + L4 of the cell's diagonal, which K[] carries along.
		const int rowc = qlen - 1 - i, rc = rowc - cb, g_row = frank(rowc);
		int acc[CPL];
#pragma unroll
		for (int jj = 0; jj < CPL; ++jj) {
			const int xt1 = jj ? X[jj ? jj - 1 : 0] : xl, vt1 = jj ? V[jj ? jj - 1 : 0] : vl, x2t1 = jj ? X2[jj ? jj - 1 : 0] : x2l;
			const int sc = *(const int *)((const char *)sc_lut + (TC[jj] | qc4));
			const int ut = U[jj];
			int za = xt1 + vt1, zb = Y[jj] + ut, za2 = x2t1 + vt1, zb2 = Y2[jj] + ut;
			int m = max(max(sc, za), zb);
			m = max(max(m, za2), zb2);
			const int z = min(m, z_cap) & ~7;
			const int un = z - vt1, vn = z - ut;
			const int zq = z - q_m8, zq2 = z - q2_m8;
			za -= zq, zb -= zq, za2 -= zq2, zb2 -= zq2;                // negative <=> the gap is not extended (:188-213)
			int a = m;                                                // direction byte: tag in bits 4-6, the four signs below it
			a = (int)__builtin_amdgcn_alignbit((unsigned)a, (unsigned)za, 31);
			a = (int)__builtin_amdgcn_alignbit((unsigned)a, (unsigned)zb, 31);
			a = (int)__builtin_amdgcn_alignbit((unsigned)a, (unsigned)za2, 31);
			a = (int)__builtin_amdgcn_alignbit((unsigned)a, (unsigned)zb2, 31);
			acc[jj] = a;
			const int hn = H[jj] + vn;                                 // exact H, times 8 like the differences (:316-351), see h_above
			int key = 0;
			if (!LEAN) {
				const int low = ((jj - K[jj]) & 0x4000) | (jj <= rc ? G[jj] : g_row);   // 0x7fff - rank
				key = (int)((unsigned)hn << 13) | low;                   // H in the upper half (bits 13-15 of the shifted value are zero: hn is a multiple of 8)
			}
			if (!TEAM_MASKED || act) {
				U[jj] = un, V[jj] = vn;
				X[jj] = max(za, -5) + cx, Y[jj] = max(zb, -6) + cx;
				X2[jj] = max(za2, -7) + cx2, Y2[jj] = max(zb2, -8) + cx2;
				H[jj] = hn;
			}
			if (!LEAN) M[jj] = max(M[jj], (act & inr[jj]) ? key : kNone);
		}
		// anti-diagonal i + cb is complete as far as this lane and the ones right of it go: on to the left neighbour, or -- first lane --
		// merged with what the strips before left
		const int out = LEAN ? 0 : M[0];
		if (!LEAN && ql == 0) at4(uD, c0 + k) = max(out, d_row);
		if (!LEAN) {
			const int d_in = i + cb + CPL;                              // the diagonal that enters at the last column with the next row
			const int st_in = max(0, d_in - qlen + 1), en_in = min(tlen - 1, d_in);
#pragma unroll
			for (int jj = 0; jj + 1 < CPL; ++jj) M[jj] = M[jj + 1], K[jj] = K[jj + 1] + 0;
			M[CPL - 1] = kNone, K[CPL - 1] = st_in + ((en_in - st_in) & ~3) - cb;
		}
		// one byte per cell, the lane's CPL cells of a step side by side: [step][lane][cell]; stored by the NEXT step's cluster (above),
		// so that no store stands right in front of the step's wait
#pragma unroll
		for (int g = 0; g < CPL; g += 4) {
			const unsigned lo = __builtin_amdgcn_perm((unsigned)acc[g + 1], (unsigned)acc[g], 0x0c0c0400u);
			const unsigned hi = __builtin_amdgcn_perm((unsigned)acc[g + 3], (unsigned)acc[g + 2], 0x04000c0cu);
			dirw[g >> 2] = lo | hi;
		}
		// what crosses into the next strip -- v, x, x2 of the strip's last column, one dword -- or, in the alignment's last strip, H of the
		// last target column (cell (i, tlen - 1), see below): one value per lane and step, stored with the next step's cluster like dirw
		// (CARRY 0: stored here, at the end of the step, and waited for by the next step moments later)
		if (CARRY) {
			unsigned c = 0;                                             // (set afresh in every step: nothing rides round the loop in it)
			if (eown) c = (((unsigned)V[CPL - 1] >> 3) & 0xffu) | ((((unsigned)X[CPL - 1] >> 3) & 0xffu) << 8) | ((((unsigned)X2[CPL - 1] >> 3) & 0xffu) << 16);
			if (own) {
				int hx = H[CPL - 1];
#pragma unroll
				for (int u = CPL - 2; u >= 0; --u) hx = jx == u ? H[u] : hx;
				c = (unsigned)(hx >> 3);
			}
			carry = c;
		} else {
			if (eown & act)
				at4(Eout, i) = (int)((((unsigned)V[CPL - 1] >> 3) & 0xffu) | ((((unsigned)X[CPL - 1] >> 3) & 0xffu) << 8) | ((((unsigned)X2[CPL - 1] >> 3) & 0xffu) << 16));
			if (own & act) {
				int hx = H[CPL - 1];
#pragma unroll
				for (int u = CPL - 2; u >= 0; --u) hx = jx == u ? H[u] : hx;
				atD2(i + tlen - 1) = (short)(hx >> 3);
			}
		}
		// H at the band ends, for the maximum's tie rule / mte / mqe / score: cell (r - en0, en0) is in the top row (r < tlen) or in the last
		// column, cell (qlen - 1, r - qlen + 1) in the last row
		if (TEAM_TOPROW && i == 0) {
#pragma unroll
			for (int jj = 0; jj < CPL; ++jj) if (inr[jj]) atD2(cb + jj) = (short)(H[jj] >> 3);
		}
		if (k >= k_last && i == qlen - 1) {                            // (k_last: the first step in which a lane of this wavefront is in its last row)
#pragma unroll
			for (int jj = 0; jj < CPL; ++jj) if (inr[jj]) atD3(qlen - 1 + cb + jj) = (short)(H[jj] >> 3);
		}
		out_prev = out;
